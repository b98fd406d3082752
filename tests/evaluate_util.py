"""Shared helpers of the tests of the evaluation at caller-given times (test_evaluate_host.py, test_gpu_evaluate.py): the
fixtures, the CPU harness of csrc/mrs_tg_evaluate.hpp, and a plain-Python restatement of the locate rule."""
import functools
import math

import numpy as np

from tests import host_harness as hh

ROOT = hh.ROOT
load_cases = functools.partial(hh.load_cases, "evaluate_cases.json")
load_composite_cases = functools.partial(hh.load_cases, "evaluate_composite_cases.json")
build_harness = functools.partial(hh.build, "evaluate_harness.cpp")   # (tmp_path, sanitize=False)
N, D, ORDERS = 10, 4, 5


def gradient_cases():
    return [c for c in load_cases() if not c.get("forward")]


def forward_cases():
    return [c for c in load_cases() if c.get("forward")]


def query_array(case):
    """the case's query times as doubles (null in the JSON = NaN)"""
    return np.array([np.nan if t is None else t for t in case["query_times"]], dtype=np.float64)


def locate(seg_times, t):
    """The rule of DESIGN.md section 7c in Python floats (IEEE doubles): (segment, tau), (-1, 0.0) = out of range."""
    acc = 0.0
    sums = []
    for T in seg_times:
        acc = acc + float(T)
        sums.append(acc)
    t = float(t)
    if not (t >= 0.0) or acc != acc:
        return -1, 0.0
    stop = None
    for i, a in enumerate(sums):
        if a > t:
            stop = i
            break
    if stop is None:
        if t > acc:
            return -1, 0.0
        stop = len(sums) - 1
    start = sums[stop] - float(seg_times[stop])
    return stop, t - start


def run_harness(exe, problems, env=None):
    """problems: dicts with seg_times [S], coeffs [S][4][10], query_times [Q], n_orders, grad_states [Q][n_orders][4] (default
    zeros), optional status (default 1).
    -> list of dicts query_segment [Q], query_local_time [Q], states [Q][n_orders][4], grad_coeffs [S][4][10],
    grad_seg_times [S], grad_query_times [Q]"""
    lines = []
    for p in problems:
        S, Q, no = len(p["seg_times"]), len(p["query_times"]), p["n_orders"]
        G = p.get("grad_states")
        G = np.zeros((Q, no, D)) if G is None else np.asarray(G, dtype=np.float64).reshape(Q, no, D)
        lines.append("%d %d %d %d %s %s %s %s\n" % (S, no, Q, p.get("status", 1), hh.fmt(p["seg_times"]), hh.fmt(p["coeffs"]),
                                                     hh.fmt(p["query_times"]), hh.fmt(G)))
    out = hh.run(exe, lines, len(problems), timeout=900, env=env)
    res = []
    for p, line in zip(problems, out):
        S, Q, no = len(p["seg_times"]), len(p["query_times"]), p["n_orders"]
        x = line.split()
        per = 2 + no * D
        assert len(x) == Q * per + S * D * N + S + Q, (len(x), Q, S)
        head = np.array([float(v) for v in x[:Q * per]]).reshape(Q, per)
        rest = np.array([float(v) for v in x[Q * per:]])
        res.append(dict(query_segment=head[:, 0].astype(np.int64), query_local_time=head[:, 1].copy(),
                        states=head[:, 2:].reshape(Q, no, D).copy(), grad_coeffs=rest[:S * D * N].reshape(S, D, N),
                        grad_seg_times=rest[S * D * N:S * D * N + S], grad_query_times=rest[S * D * N + S:], raw=line))
    return res


def case_problem(case, **over):
    p = dict(seg_times=case["seg_times"], coeffs=case["coeffs"], query_times=query_array(case), n_orders=case["n_orders"],
             grad_states=case.get("grad_states"))
    p.update(over)
    return p


def fixture_error(case, grad_coeffs, grad_seg_times, grad_query_times):
    """|got - fixture| relative to the case's largest gradient entry (a directional case: the three directional derivatives
    relative to the largest of them)"""
    gc = np.asarray(grad_coeffs, dtype=np.float64)
    gt = np.asarray(grad_seg_times, dtype=np.float64)
    gq = np.asarray(grad_query_times, dtype=np.float64)
    if "directions" in case:
        refs = np.array([d["derivative"] for d in case["directions"]])
        got = np.array([np.sum(gc * (np.array(d["d_coeffs_sixteenths"]) / 16.0)) + np.sum(gt * np.array(d["d_seg_times"])) +
                        np.sum(gq * np.array(d["d_query_times"])) for d in case["directions"]])
        return float(np.max(np.abs(got - refs)) / np.max(np.abs(refs)))
    rc, rt, rq = np.array(case["grad_coeffs"]), np.array(case["grad_seg_times"]), np.array(case["grad_query_times"])
    scale = max(np.max(np.abs(rc)), np.max(np.abs(rt)), np.max(np.abs(rq)))
    return float(max(np.max(np.abs(gc - rc)), np.max(np.abs(gt - rt)), np.max(np.abs(gq - rq))) / scale)


def forward_error(case, states):
    """(worst |got - fixture| / largest entry of that order in the case, whether every order is within 1e-13 of it).  No
    fixture needs more than that constant (the generator prints each case's Horner rounding bound; it is kept in the
    fixture as horner_bound)."""
    ref = np.array(case["states"], dtype=np.float64)
    got = np.array(states, dtype=np.float64).copy()
    # the heading of order 0 modulo 2 pi (the fixture is not wrapped)
    d0 = got[:, 0, 3] - ref[:, 0, 3]
    got[:, 0, 3] -= 2.0 * math.pi * np.round(d0 / (2.0 * math.pi))
    worst, ok = 0.0, True
    for o in range(ref.shape[1]):
        scale = np.max(np.abs(ref[:, o, :]))
        err = float(np.max(np.abs(got[:, o, :] - ref[:, o, :])))
        ok = ok and err <= 1e-13 * scale
        worst = max(worst, err / scale)
    return worst, ok


def wrapped_in_range(states):
    h = np.asarray(states)[:, 0, 3]
    return bool(np.all(np.abs(h) <= math.pi + 1e-15))


# ------------------------------------------------------------------------------------------------------------------------
# torch restatement

def falling(j, o):
    v = 1.0
    for n in range(o):
        v *= (j - n)
    return v


def derivative_at(torch, coeffs, seg, t, o, absolute=False):
    """dense float64 Horner: the o-th derivative [K][4] (o up to 9) of the polynomials of the segments seg [K] (int64 rows of
    coeffs [sum S][4][10]) at the times t [K]; differentiable in coeffs and t.  absolute: sum_j |j!/(j-o)! c_j| |t|^(j-o)
    instead (what bounds the rounding of that chain)."""
    c = coeffs[seg]   # [K][4][10]
    if absolute:
        c, t = c.abs(), t.abs()
    acc = c[:, :, N - 1] * falling(N - 1, o)
    for j in range(N - 2, o - 1, -1):
        acc = acc * t[:, None] + c[:, :, j] * falling(j, o)
    return acc


def states_at(torch, coeffs, seg, t, n_orders=ORDERS):
    """states [K][n_orders][4] at (segment, time in segment) pairs; the heading is NOT wrapped"""
    return torch.stack([derivative_at(torch, coeffs, seg, t, o) for o in range(n_orders)], dim=1)


def local_time_expr(torch, seg_times, seg_offsets, p_idx, seg_rel, t):
    """tau = t - (sum of the times of the path's segments in front of the query's own), a differentiable expression:
    seg_times [sum S], seg_offsets [P + 1] (CSR), p_idx [K] the query's path, seg_rel [K] its segment within the path, t [K]
    the query times (tensors on seg_times' device).  The sums are taken per path."""
    dev = seg_times.device
    so = torch.as_tensor(np.asarray(seg_offsets, dtype=np.int64), device=dev)
    counts = so[1:] - so[:-1]
    cols = torch.arange(int(counts.max()), device=dev)
    inside = cols[None, :] < counts[:, None]
    rows = torch.where(inside, so[:-1, None] + cols[None, :], torch.zeros((), dtype=torch.int64, device=dev))
    Tm = torch.where(inside, seg_times[rows], torch.zeros((), dtype=seg_times.dtype, device=dev))
    before = torch.cumsum(Tm, dim=1) - Tm
    return t - before[p_idx, seg_rel]

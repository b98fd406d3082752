#!/usr/bin/env python3
"""Generate tests/golden/evaluate_cases.json and evaluate_composite_cases.json: 60-digit states of a trajectory at given
times and 60-digit gradients of a loss on them, for mrs_tg_plan_evaluate / mrs_tg_plan_evaluate_vjp.

The ground truth of the gradients is NOT the formulas of DESIGN.md section 7c: it is central differences (step 1e-20) of
L = sum G . state over an exact-arithmetic restatement of the evaluator -- the segment of the query t is the first i whose
exact cumulative time exceeds t, state[q][o][dim] the o-th derivative of that segment's polynomial at t minus the exact
prefix (the heading unwrapped: the wrap adds a constant multiple of 2 pi between seams and has derivative 1) -- in every
coefficient, every segment time and every query time.  (L is linear in the coefficients, so a difference in c[i][dim][j] is
taken over the terms of segment i and dimension dim, the only ones that move; a difference in t_q over the terms of query q.)
Upstreams are dyadic, so they are exact in double; coefficients, times and queries are taken as exact doubles.

Gradient cases: the generator asserts that every query lies at least 1e-6 s from both ends of its segment (the membership
cannot change within the step, and the double-precision rule picks the same segment).  Coefficients of solved paths at
d = 2, 3, 4 (oracle/gen_golden.py's exact_solve at Euclidean times), n_orders 1 and 5; unsorted queries with a duplicate; a
segment that holds no query; a heading that crosses pi; a 30-segment path along three random directions (d_coeffs_sixteenths:
the direction in the coefficients, in units of 1/16).

Forward-only cases ("forward": true): states to 60 digits and the expected segment of queries at exactly 0, at exactly an
interior vertex, at exactly the total as double arithmetic sums it, one ulp on either side of it, a negative and a NaN query
(null in the JSON), and a path with a zero-length segment.  The segment is the double-precision rule's (a plain restatement
here); the state is the exact polynomial of that segment at t minus the exact prefix.  horner_bound[q][o] is the rounding
bound sum_j |j!/(j-o)! c_j| |tau|^(j-o) 64 eps of the Horner chain, maximised over the dimensions.

Composite cases: L = sum G . states(solve(fv, T), T, t), with tests/golden/gen_vjp_cases.py's dense 60-digit KKT solve
(kkt_solver, imported): central differences in every fixed slot of the fixed values, every segment time and every query time
-- the chain autograd.solve -> autograd.evaluate.  One path is ill-conditioned: a segment 50 times shorter than its neighbours.

Run from the repo root:  python3 tests/golden/gen_evaluate_cases.py   (a few minutes)
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_sample_vjp_cases import coeffs_of, deriv, dyadic, ff, solved  # noqa: E402
from gen_vjp_cases import kkt_solver  # noqa: E402

mp.mp.dps = 60
N, D, B = 10, 4, 5
STEP = mp.mpf("1e-20")
MARGIN = mp.mpf("1e-6")
EPS = 2.0 ** -52
OUT = os.path.join(ROOT, "tests", "golden", "evaluate_cases.json")
OUT_COMPOSITE = os.path.join(ROOT, "tests", "golden", "evaluate_composite_cases.json")


def exact_locate(tm, t):
    """(segment, time in segment) by the exact cumulative times; t in [0, sum T]"""
    cum = mp.mpf(0)
    for i, T in enumerate(tm):
        if cum + T > t:
            return i, t - cum
        cum += T
    assert t == cum
    return len(tm) - 1, t - (cum - tm[-1])


def double_locate(times, t):
    """the rule in doubles, as DESIGN.md section 7c states it: (segment or -1, tau)"""
    acc, stop = 0.0, None
    sums = []
    for T in times:
        acc += T
        sums.append(acc)
    if not (t >= 0.0) or acc != acc:
        return -1, 0.0
    for i, a in enumerate(sums):
        if a > t:
            stop = i
            break
    if stop is None:
        if t > acc:
            return -1, 0.0
        stop = len(times) - 1
    return stop, t - (sums[stop] - times[stop])


def loss(cm, tm, qm, G, n_orders, only=None, only_query=None):
    """sum G . state; only = (segment, dim): just that segment's and dimension's terms; only_query: just that query's"""
    s = mp.mpf(0)
    for q, t in enumerate(qm):
        if only_query is not None and q != only_query:
            continue
        i, tau = exact_locate(tm, t)
        if only is not None and i != only[0]:
            continue
        for dim in range(D):
            if only is not None and dim != only[1]:
                continue
            for o in range(n_orders):
                g = G[q][o][dim]
                if g != 0.0:
                    s += mp.mpf(g) * deriv(cm[i][dim], tau, o)
    return s


def check_queries(name, times, queries):
    """the finite-difference condition and the agreement of the double-precision rule; -> segments, local times"""
    tm = [mp.mpf(float(t)) for t in times]
    segs, taus = [], []
    for t in queries:
        i, tau = exact_locate(tm, mp.mpf(float(t)))
        assert tau >= MARGIN and tm[i] - tau >= MARGIN, (name, t, i, tau)
        di, dtau = double_locate([float(x) for x in times], float(t))
        assert di == i and abs(dtau - tau) < 1e-12, (name, t)
        segs.append(i)
        taus.append(float(tau))
    return segs, taus


def record(name, coeffs, times, queries, n_orders, seed, directional=0):
    S, Q = len(times), len(queries)
    rng = np.random.default_rng(seed)
    c = np.asarray(coeffs, dtype=np.float64)
    segs, taus = check_queries(name, times, queries)
    G = dyadic(rng, (Q, n_orders, D), 64.0)
    cm = [[[mp.mpf(float(c[i, k, j])) for j in range(N)] for k in range(D)] for i in range(S)]
    tm = [mp.mpf(float(t)) for t in times]
    qm = [mp.mpf(float(t)) for t in queries]
    rec = dict(name=name, n_orders=n_orders, seg_times=[float(t) for t in times], coeffs=c.tolist(),
               query_times=[float(t) for t in queries], grad_states=G.tolist(), query_segment=segs, query_local_time=taus,
               step=float(STEP))
    if directional:
        dirs = []
        for _ in range(directional):
            dT = [float(x) for x in (rng.integers(-8, 9, size=S) / 16.0) * np.asarray(times)]
            dq = [float(x) for x in rng.integers(-8, 9, size=Q) / 16.0]
            dc16 = rng.integers(-16, 17, size=(S, D, N))
            dc = dc16 / 16.0
            vals = []
            for sgn in (1, -1):
                t = [tm[i] + sgn * STEP * mp.mpf(dT[i]) for i in range(S)]
                qq = [qm[i] + sgn * STEP * mp.mpf(dq[i]) for i in range(Q)]
                cc = [[[cm[i][k][j] + sgn * STEP * mp.mpf(float(dc[i, k, j])) for j in range(N)] for k in range(D)] for i in range(S)]
                vals.append(loss(cc, t, qq, G, n_orders))
            dirs.append(dict(d_seg_times=dT, d_query_times=dq, d_coeffs_sixteenths=dc16.tolist(),
                             derivative=float((vals[0] - vals[1]) / (2 * STEP))))
        rec["directions"] = dirs
        return rec
    gc = np.zeros((S, D, N))
    for i in range(S):
        for k in range(D):
            for j in range(N):
                keep = cm[i][k][j]
                cm[i][k][j] = keep + STEP
                lp = loss(cm, tm, qm, G, n_orders, only=(i, k))
                cm[i][k][j] = keep - STEP
                lm = loss(cm, tm, qm, G, n_orders, only=(i, k))
                cm[i][k][j] = keep
                gc[i, k, j] = float((lp - lm) / (2 * STEP))
    gt = []
    for i in range(S):
        tp, tq = list(tm), list(tm)
        tp[i] += STEP
        tq[i] -= STEP
        gt.append(float((loss(cm, tp, qm, G, n_orders) - loss(cm, tq, qm, G, n_orders)) / (2 * STEP)))
    gq = []
    for q in range(Q):
        qp, qn = list(qm), list(qm)
        qp[q] += STEP
        qn[q] -= STEP
        gq.append(float((loss(cm, tm, qp, G, n_orders, only_query=q) - loss(cm, tm, qn, G, n_orders, only_query=q)) / (2 * STEP)))
    rec["grad_coeffs"] = gc.tolist()
    rec["grad_seg_times"] = gt
    rec["grad_query_times"] = gq
    return rec


def random_queries(rng, times, count, avoid=()):
    """count query times in (0, sum T), each at least 1e-3 s inside its segment, none in the segments `avoid`"""
    edges = np.concatenate([[0.0], np.cumsum(times)])
    out = []
    while len(out) < count:
        t = float(rng.uniform(0.0, edges[-1]))
        i = int(np.searchsorted(edges, t, side="right")) - 1
        if i in avoid or t - edges[i] < 1e-3 or edges[i + 1] - t < 1e-3:
            continue
        out.append(t)
    return out


def forward_record(name, coeffs, times, queries, n_orders):
    """states to 60 digits at the double-precision rule's segment; queries may hold None (NaN)"""
    c = np.asarray(coeffs, dtype=np.float64)
    S = len(times)
    cm = [[[mp.mpf(float(c[i, k, j])) for j in range(N)] for k in range(D)] for i in range(S)]
    tm = [mp.mpf(float(t)) for t in times]
    segs, states, bounds = [], [], []
    for t in queries:
        tf = float("nan") if t is None else float(t)
        i, dtau = double_locate([float(x) for x in times], tf)
        segs.append(i)
        if i < 0:
            states.append(np.zeros((n_orders, D)).tolist())
            bounds.append([0.0] * n_orders)
            continue
        tau = mp.mpf(tf) - sum(tm[:i], mp.mpf(0))
        assert abs(tau - dtau) < 1e-12
        states.append([[float(deriv(cm[i][dim], tau, o)) for dim in range(D)] for o in range(n_orders)])
        bounds.append([max(float(sum(abs(ff(j, o) * cm[i][dim][j]) * abs(tau) ** (j - o) for j in range(o, N))) for dim in range(D))
                       * 64 * EPS for o in range(n_orders)])
    return dict(name=name, forward=True, n_orders=n_orders, seg_times=[float(t) for t in times], coeffs=c.tolist(),
                query_times=[None if t is None else float(t) for t in queries], query_segment=segs, states=states,
                horner_bound=bounds)


def double_sums(times):
    acc, out = 0.0, []
    for t in times:
        acc += t
        out.append(acc)
    return out


def cases():
    out = []
    for name, S, d, seed, no, Q in (("d2_s3_o5", 3, 2, 900, 5, 7), ("d3_s5_o1", 5, 3, 901, 1, 9), ("d4_s4_o5", 4, 4, 902, 5, 8),
                                    ("d4_s6_o1", 6, 4, 903, 1, 10), ("d3_s4_o5", 4, 3, 904, 5, 6), ("d2_s4_o1", 4, 2, 905, 1, 8)):
        m, v, t = solved(S, seed, d)
        rng = np.random.default_rng(seed + 50)
        out.append(record(name, coeffs_of(m, v, t, d), t, sorted(random_queries(rng, t, Q)), no, seed))
    # any order, one time asked twice
    m, v, t = solved(5, 910, 4)
    rng = np.random.default_rng(960)
    q = random_queries(rng, t, 8)
    q = [q[3]] + q   # (random_queries returns them unsorted)
    assert q != sorted(q) and len(set(q)) == len(q) - 1
    out.append(record("unsorted_duplicate_o5", coeffs_of(m, v, t, 4), t, q, 5, 910))
    # a segment nobody asks about, with queries on both sides of it
    m, v, t = solved(5, 911, 3)
    rng = np.random.default_rng(961)
    edges = [0.0] + double_sums(t)
    q = random_queries(rng, t, 5, avoid=(2,)) + [edges[i] + float(rng.uniform(0.2, 0.8)) * t[i] for i in (0, 1, 3, 4)]
    rec =record("empty_segment_o5", coeffs_of(m, v, t, 3), t, q, 5, 911)
    assert 2 not in rec["query_segment"] and {1, 3} <= set(rec["query_segment"])
    out.append(rec)
    # the heading crosses pi between two queries
    m, v, t = solved(4, 912, 4, headings=np.linspace(2.6, 3.8, 5))
    c = coeffs_of(m, v, t, 4)
    rng = np.random.default_rng(962)
    rec = record("heading_crosses_pi_o5", c, t, sorted(random_queries(rng, t, 10)), 5, 912)
    yaw = [float(sum(c[i, 3, j] * tt ** j for j in range(N))) for i, tt in zip(rec["query_segment"], rec["query_local_time"])]
    assert any(a < np.pi < b for a, b in zip(yaw[:-1], yaw[1:])), yaw
    out.append(rec)
    m, v, t = solved(30, 940, 4)
    rng = np.random.default_rng(990)
    out.append(record("seg30_directional", coeffs_of(m, v, t, 4), t, random_queries(rng, t, 24), 1, 940, directional=3))
    # forward only: the ends of the range, a vertex, out of range
    m, v, t = solved(4, 920, 4)
    c = coeffs_of(m, v, t, 4)
    sums = double_sums(t)
    total = sums[-1]
    q = [0.0, sums[1], total, float(np.nextafter(total, np.inf)), float(np.nextafter(total, -np.inf)), -0.5, None, 0.5 * sums[0], -0.0]
    rec = forward_record("forward_edges_o5", c, t, q, 5)
    assert rec["query_segment"] == [0, 2, 3, -1, 3, -1, -1, 0, 0], rec["query_segment"]
    out.append(rec)
    out.append(forward_record("forward_edges_o1", c, t, q, 1))
    # a zero-length segment is skipped: the query on its two coinciding vertices belongs to the segment behind it
    t0 = list(t)
    t0[1] = 0.0
    s0 = double_sums(t0)
    q = [s0[0], 0.5 * s0[0], s0[0] + 0.25 * t0[2], s0[-1], float(np.nextafter(s0[0], -np.inf))]
    rec = forward_record("zero_length_segment_o5", c, t0, q, 5)
    assert rec["query_segment"] == [2, 0, 2, 3, 0], rec["query_segment"]
    out.append(rec)
    return out


def composite_record(name, m, v, t, d, queries, n_orders, seed):
    S, Q = len(t), len(queries)
    n_all = B * (S + 1)
    rng = np.random.default_rng(seed)
    tm = [mp.mpf(float(x)) for x in t]
    qm = [mp.mpf(float(x)) for x in queries]
    vflat = np.asarray(v, dtype=np.float64).reshape(n_all, D)
    vm = [[mp.mpf(float(vflat[i, k])) for k in range(D)] for i in range(n_all)]
    flat = np.asarray(m).reshape(-1)
    solve0 = kkt_solver(m, tm, d)
    segs, _ = check_queries(name, t, queries)
    G = dyadic(rng, (Q, n_orders, D), 64.0)

    def L_at(tt, vv, qq=qm, only_query=None):
        c, _ = (solve0 if tt is tm else kkt_solver(m, tt, d))(vv)
        return loss(c, tt, qq, G, n_orders, only_query=only_query)

    gt = []
    for i in range(S):
        tp, tq = list(tm), list(tm)
        tp[i] += STEP
        tq[i] -= STEP
        gt.append(float((L_at(tp, vm) - L_at(tq, vm)) / (2 * STEP)))
    gv = np.zeros((n_all, D))
    for i in range(n_all):
        if not flat[i]:
            continue
        for k in range(D):
            vp, vq = [row[:] for row in vm], [row[:] for row in vm]
            vp[i][k] += STEP
            vq[i][k] -= STEP
            gv[i, k] = float((L_at(tm, vp) - L_at(tm, vq)) / (2 * STEP))
    c0, _ = solve0(vm)
    gq = []
    for q in range(Q):
        qp, qn = list(qm), list(qm)
        qp[q] += STEP
        qn[q] -= STEP
        gq.append(float((loss(c0, tm, qp, G, n_orders, only_query=q) - loss(c0, tm, qn, G, n_orders, only_query=q)) / (2 * STEP)))
    return dict(name=name, derivative_to_optimize=d, n_orders=n_orders, fixed_mask=np.asarray(m).astype(int).tolist(),
                fixed_values=np.asarray(v, dtype=np.float64).tolist(), seg_times=[float(x) for x in t],
                query_times=[float(x) for x in queries], query_segment=segs, grad_states=G.tolist(), grad_seg_times=gt,
                grad_query_times=gq, grad_fixed_values=gv.reshape(S + 1, B, D).tolist(), step=float(STEP))


def composite_cases():
    out = []
    for name, S, d, seed, no in (("d3_s4", 4, 3, 950, 1), ("d4_s5", 5, 4, 951, 5)):
        m, v, t = solved(S, seed, d)
        rng = np.random.default_rng(seed + 20)
        out.append(composite_record(name, m, v, t, d, random_queries(rng, t, 8), no, seed))
    m, v, t = solved(6, 860, 4)
    t[3] = 0.5 * (t[2] + t[4]) / 50.0
    rng = np.random.default_rng(980)
    q = random_queries(rng, t, 7, avoid=(3,)) + [float(sum(t[:3]) + 0.5 * t[3])]
    out.append(composite_record("ratio50", m, v, t, 4, q, 1, 860))
    return out


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("all", "cases"):
        cs = cases()
        with open(OUT, "w") as f:
            json.dump(dict(generator="tests/golden/gen_evaluate_cases.py", mp_dps=60, cases=cs), f)
        print("wrote", len(cs), "cases to", OUT)
        for c in cs:
            if c.get("forward"):
                print("  %s: largest Horner bound %.2e" % (c["name"], max(max(b) for b in c["horner_bound"])))
    if which in ("all", "composite"):
        cc = composite_cases()
        with open(OUT_COMPOSITE, "w") as f:
            json.dump(dict(generator="tests/golden/gen_evaluate_cases.py", mp_dps=60, cases=cc), f)
        print("wrote", len(cc), "composite cases to", OUT_COMPOSITE)


if __name__ == "__main__":
    main()

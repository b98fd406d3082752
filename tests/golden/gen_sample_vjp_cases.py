#!/usr/bin/env python3
"""Generate tests/golden/sample_vjp_cases.json and sample_vjp_composite_cases.json: 60-digit gradients of a loss on the
samples of a trajectory, for mrs_tg_plan_sample_states_vjp.

The ground truth is NOT the formulas of DESIGN.md section 7b: it is central differences (step 1e-20) of L = sum G . state
over an exact-arithmetic restatement of the sampler -- sample k at k dt, its segment found from the cumulative times with the
walk's `>` carry rule, state[k][o][dim] the o-th derivative of the segment's polynomial (the heading unwrapped: the wrap adds a
constant multiple of 2 pi between seams and has derivative 1) -- in every coefficient and every segment time.  (L is linear
in the coefficients, so a difference in c[i][dim][j] is taken over the terms of segment i and dimension dim, the only ones that
move.)  Upstreams are dyadic, so they are exact in double; coefficients and times are taken as exact doubles.

For every case the generator asserts what makes a finite difference meaningful: every sample k >= 1 lies at least 1e-6 s from
both ends of its segment and sum T - (n - 1) dt >= 1e-6; and that the double-precision walk assigns the same n (the oracle's
sample_trajectory count) and the same segments (a serial restatement of the accumulate-and-carry loop).

Cases (coefficients of solved paths at d = 2, 3, 4; oracle/gen_golden.py's exact_solve at Euclidean times): dt 0.2 and 0.5;
n_orders 1 and 5; a segment shorter than dt that holds no sample; a segment that holds exactly one; a heading that crosses pi
between two samples; capacity < n (overflow: the ground truth is over the first `capacity` samples); a 30-segment path along
three random directions (d_coeffs_sixteenths: the direction in the coefficients, in units of 1/16).

Composite cases: L = sum G . samples(solve(fv, T), T), positions + heading, with tests/golden/gen_vjp_cases.py's dense 60-digit
KKT solve (kkt_solver, imported): central differences in every fixed slot of the fixed values and in every segment time -- the
chain autograd.solve -> autograd.sample.  One path is ill-conditioned: a segment 50 times shorter than its neighbours.

Run from the repo root:  python3 tests/golden/gen_sample_vjp_cases.py   (a few minutes)
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mrs_uav_trajectory_generation_amd import problem as pr  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from oracle.gen_golden import euclid_times, exact_solve  # noqa: E402
from gen_vjp_cases import kkt_solver  # noqa: E402

mp.mp.dps = 60
N, D, B = 10, 4, 5
STEP = mp.mpf("1e-20")
MARGIN = mp.mpf("1e-6")
OUT = os.path.join(ROOT, "tests", "golden", "sample_vjp_cases.json")
OUT_COMPOSITE = os.path.join(ROOT, "tests", "golden", "sample_vjp_composite_cases.json")


def ff(j, o):
    v = 1
    for n in range(o):
        v *= j - n
    return v


def deriv(c, t, o):
    """o-th derivative of sum c_j t^j (mpf)"""
    return sum(ff(j, o) * c[j] * t ** (j - o) for j in range(o, N))


def exact_walk(times, dt, limit=None):
    """[(segment, time in segment)] of the samples k dt < sum T, the first `limit` of them; and their number n"""
    total = sum(times)
    out, n, i, cum = [], 0, 0, mp.mpf(0)
    while n * dt < total:
        tin = n * dt - cum
        while tin > times[i]:
            cum += times[i]
            tin -= times[i]
            i += 1
        if limit is None or n < limit:
            out.append((i, tin))
        n += 1
    return out, n


def double_walk(times, dt, limit):
    """the accumulate-and-carry loop in doubles: [(segment, time in segment)], n (stops at limit + 1)"""
    t_end = 0.0
    for t in times:
        t_end += t
    out, n, i, tin, acc = [], 0, 0, 0.0, 0.0
    while acc < t_end:
        while i < len(times) and tin > times[i]:
            tin -= times[i]
            i += 1
        if i >= len(times):
            break
        if n < limit:
            out.append((i, tin))
        n += 1
        if n > limit:
            break
        tin += dt
        acc += dt
    return out, n


def loss(cm, tm, dt, G, n_orders, limit, only=None):
    """sum G . state over the first `limit` samples; only = (segment, dim): just that segment's and dimension's terms"""
    walk, _ = exact_walk(tm, dt, limit)
    s = mp.mpf(0)
    for k, (i, t) in enumerate(walk):
        if only is not None and i != only[0]:
            continue
        for dim in range(D):
            if only is not None and dim != only[1]:
                continue
            for o in range(n_orders):
                g = G[k][o][dim]
                if g != 0.0:
                    s += mp.mpf(g) * deriv(cm[i][dim], t, o)
    return s


def dyadic(rng, shape, denom):
    return (rng.integers(-64, 65, size=shape) / denom).astype(np.float64)


def check_walk(name, times, dt, coeffs, capacity):
    """the finite-difference condition and the agreement of the double-precision walk; -> (n, segments, times in segment)"""
    tm = [mp.mpf(float(t)) for t in times]
    dtm = mp.mpf(float(dt))
    walk, n = exact_walk(tm, dtm)
    for k, (i, t) in enumerate(walk):
        if k >= 1:
            assert t >= MARGIN and tm[i] - t >= MARGIN, (name, k, i, t)
    assert sum(tm) - (n - 1) * dtm >= MARGIN, name
    _, n_oracle = po.sample_trajectory(np.asarray(coeffs), np.asarray(times, dtype=np.float64), float(dt), 0, 1 << 16)
    assert n_oracle == n, (name, n_oracle, n)
    dwalk, dn = double_walk([float(t) for t in times], float(dt), 1 << 16)
    assert dn == n and [i for i, _ in dwalk] == [i for i, _ in walk], name
    for (_, td), (_, te) in zip(dwalk, walk):
        assert abs(td - te) < 1e-9, name
    lim = min(n, capacity)
    return n, [i for i, _ in walk[:lim]], [float(t) for _, t in walk[:lim]]


def record(name, coeffs, times, dt, n_orders, seed, capacity=None, directional=0):
    S = len(times)
    rng = np.random.default_rng(seed)
    c = np.asarray(coeffs, dtype=np.float64)
    n, segs, tins = check_walk(name, times, dt, c, 1 << 16 if capacity is None else capacity)
    capacity = n + 3 if capacity is None else capacity
    rows = min(n, capacity)
    G = dyadic(rng, (rows, n_orders, D), 64.0)
    cm = [[[mp.mpf(float(c[i, k, j])) for j in range(N)] for k in range(D)] for i in range(S)]
    tm = [mp.mpf(float(t)) for t in times]
    dtm = mp.mpf(float(dt))
    rec = dict(name=name, n_orders=n_orders, dt=float(dt), capacity=int(capacity), seg_times=[float(t) for t in times],
               coeffs=c.tolist(), grad_states=G.tolist(), n_samples=int(min(n, capacity + 1)), n_exact=int(n),
               sample_segment=segs, sample_time=tins, step=float(STEP))
    if directional:
        dirs = []
        for _ in range(directional):
            dT = [float(x) for x in (rng.integers(-8, 9, size=S) / 16.0) * np.asarray(times)]
            dc16 = rng.integers(-16, 17, size=(S, D, N))
            dc = dc16 / 16.0
            vals = []
            for sgn in (1, -1):
                t = [tm[i] + sgn * STEP * mp.mpf(dT[i]) for i in range(S)]
                cc = [[[cm[i][k][j] + sgn * STEP * mp.mpf(float(dc[i, k, j])) for j in range(N)] for k in range(D)] for i in range(S)]
                vals.append(loss(cc, t, dtm, G, n_orders, rows))
            dirs.append(dict(d_seg_times=dT, d_coeffs_sixteenths=dc16.tolist(), derivative=float((vals[0] - vals[1]) / (2 * STEP))))
        rec["directions"] = dirs
        return rec
    gc = np.zeros((S, D, N))
    for i in range(S):
        for k in range(D):
            for j in range(N):
                keep = cm[i][k][j]
                cm[i][k][j] = keep + STEP
                lp = loss(cm, tm, dtm, G, n_orders, rows, only=(i, k))
                cm[i][k][j] = keep - STEP
                lm = loss(cm, tm, dtm, G, n_orders, rows, only=(i, k))
                cm[i][k][j] = keep
                gc[i, k, j] = float((lp - lm) / (2 * STEP))
    gt = []
    for i in range(S):
        tp, tq = list(tm), list(tm)
        tp[i] += STEP
        tq[i] -= STEP
        gt.append(float((loss(cm, tp, dtm, G, n_orders, rows) - loss(cm, tq, dtm, G, n_orders, rows)) / (2 * STEP)))
    rec["grad_coeffs"] = gc.tolist()
    rec["grad_seg_times"] = gt
    return rec


def solved(n_seg, seed, d, times=None, headings=None):
    """coefficients (rounded to double) of the exact solve of a random box path at Euclidean (or the given) times"""
    wp0 = pr.random_box_waypoints(n_seg, seed)
    if headings is not None:
        wp0 = np.array(wp0, dtype=np.float64)
        wp0[:, 3] = headings
    wp, m, v = pr.build_vertices(wp0, d)
    t = [float(x) for x in (euclid_times(wp, pr.DEFAULT_LIMITS) if times is None else times)]
    return m, v, t


def coeffs_of(m, v, t, d):
    ce, _, _, _ = exact_solve(m, v, t, d)
    return np.array([[[float(x) for x in dim] for dim in seg] for seg in ce])


def cases():
    out = []
    for name, S, d, seed, dt, no in (("d2_s3_dt02_o5", 3, 2, 800, 0.2, 5), ("d3_s5_dt02_o1", 5, 3, 801, 0.2, 1),
                                     ("d4_s4_dt05_o5", 4, 4, 802, 0.5, 5), ("d4_s6_dt05_o1", 6, 4, 803, 0.5, 1)):
        m, v, t = solved(S, seed, d)
        out.append(record(name, coeffs_of(m, v, t, d), t, dt, no, seed))
    # a segment shorter than dt between two samples: it starts 0.1 s behind a sample and lasts 0.05 s
    m, v, t = solved(5, 810, 4)
    dt = 0.2
    start = float(np.floor((t[0] + t[1]) / dt)) * dt + 0.1
    t[1] = start - t[0]
    t[2] = 0.05
    rec = record("short_segment_no_sample_o5", coeffs_of(m, v, t, 4), t, dt, 5, 810)
    assert 2 not in rec["sample_segment"] and 1 in rec["sample_segment"] and 3 in rec["sample_segment"]
    out.append(rec)
    # a segment that holds exactly one sample: it starts 0.05 s before a sample and lasts 0.1 s
    m, v, t = solved(5, 811, 3)
    start = float(np.floor((t[0] + t[1]) / dt)) * dt - 0.05
    t[1] = start - t[0]
    t[2] = 0.1
    rec = record("one_sample_segment_o1", coeffs_of(m, v, t, 3), t, dt, 1, 811)
    assert rec["sample_segment"].count(2) == 1
    out.append(rec)
    # the heading crosses pi between two samples
    m, v, t = solved(4, 812, 4, headings=np.linspace(2.6, 3.8, 5))
    c = coeffs_of(m, v, t, 4)
    rec = record("heading_crosses_pi_o5", c, t, 0.5, 5, 812)
    yaw = [float(sum(c[i, 3, j] * tt ** j for j in range(N))) for i, tt in zip(rec["sample_segment"], rec["sample_time"])]
    assert any(a < np.pi < b for a, b in zip(yaw[:-1], yaw[1:])), yaw
    out.append(rec)
    # more samples than fit
    m, v, t = solved(4, 813, 4)
    c = coeffs_of(m, v, t, 4)
    _, n_all = exact_walk([mp.mpf(x) for x in t], mp.mpf(dt))
    rec = record("overflow_o5", c, t, dt, 5, 813, capacity=n_all // 2)
    assert rec["n_samples"] == rec["capacity"] + 1 and len(rec["grad_states"]) == rec["capacity"]
    out.append(rec)
    m, v, t = solved(30, 840, 4)
    out.append(record("seg30_directional", coeffs_of(m, v, t, 4), t, 0.5, 1, 840, directional=3))
    return out


def composite_record(name, m, v, t, d, dt, seed):
    S = len(t)
    n_all = B * (S + 1)
    rng = np.random.default_rng(seed)
    tm = [mp.mpf(float(x)) for x in t]
    dtm = mp.mpf(float(dt))
    vflat = np.asarray(v, dtype=np.float64).reshape(n_all, D)
    vm = [[mp.mpf(float(vflat[i, k])) for k in range(D)] for i in range(n_all)]
    flat = np.asarray(m).reshape(-1)
    solve0 = kkt_solver(m, tm, d)
    c0, _ = solve0(vm)
    c0f = np.array([[[float(x) for x in dim] for dim in seg] for seg in c0])
    n, segs, tins = check_walk(name, t, dt, c0f, 1 << 16)
    G = dyadic(rng, (n, 1, D), 64.0)

    def L_at(tt, vv):
        c, _ = (solve0 if tt is tm else kkt_solver(m, tt, d))(vv)
        return loss(c, tt, dtm, G, 1, n)

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
    return dict(name=name, derivative_to_optimize=d, dt=float(dt), capacity=int(n + 3), fixed_mask=np.asarray(m).astype(int).tolist(),
                fixed_values=np.asarray(v, dtype=np.float64).tolist(), seg_times=[float(x) for x in t], n_samples=int(n),
                sample_segment=segs, grad_samples=G.reshape(n, D).tolist(), grad_seg_times=gt,
                grad_fixed_values=gv.reshape(S + 1, B, D).tolist(), step=float(STEP))


def composite_cases():
    out = []
    for name, S, d, seed in (("d3_s4", 4, 3, 850), ("d4_s5", 5, 4, 851)):
        m, v, t = solved(S, seed, d)
        out.append(composite_record(name, m, v, t, d, 0.2, seed))
    m, v, t = solved(6, 860, 4)
    t[3] = 0.5 * (t[2] + t[4]) / 50.0
    out.append(composite_record("ratio50", m, v, t, 4, 0.2, 860))
    return out


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("all", "cases"):
        cs = cases()
        with open(OUT, "w") as f:
            json.dump(dict(generator="tests/golden/gen_sample_vjp_cases.py", mp_dps=60, cases=cs), f)
        print("wrote", len(cs), "cases to", OUT)
    if which in ("all", "composite"):
        cc = composite_cases()
        with open(OUT_COMPOSITE, "w") as f:
            json.dump(dict(generator="tests/golden/gen_sample_vjp_cases.py", mp_dps=60, cases=cc), f)
        print("wrote", len(cc), "composite cases to", OUT_COMPOSITE)


if __name__ == "__main__":
    main()

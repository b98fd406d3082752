#!/usr/bin/env python3
"""Generate tests/golden/maxima_vjp_cases.json: 60-digit gradients of the per-segment maxima for
mrs_tg_plan_segment_maxima_vjp.

The ground truth is NOT the envelope formulas of DESIGN.md section 4d: it is central differences (step 1e-20) of the 60-digit
maximum M = max over [0, T] of |p^(k)| in every coefficient of the entry's group and in T.  The maximiser of the unperturbed
segment is found as oracle/gen_golden.py's max_magnitude finds it (sign changes of d|p^(k)|^2/dt on a fine grid, bisected),
then polished by Newton; its value is checked against max_magnitude itself (imported, unchanged).  At a perturbed point the
maximiser is polished by Newton from the unperturbed one (an end-point maximiser stays at its end point).  The coefficients
are taken as exact doubles (what the forward reads).  Every entry stores t*, M, dM/dc [4][10] (0 outside the group) and
dM/dT; an entry whose two largest local maxima tie (to 1e-30) stores the one-sided gradient of each ("alternatives").
Cases:

  * segments of solved paths at d = 2, 3, 4 (oracle/gen_golden.py's exact_solve, Euclidean times);
  * an end-point maximum (non-zero dM/dT) and a start-point maximum;
  * a constant heading (zero maximum);
  * a symmetric rest-to-rest segment whose two acceleration peaks tie.

Composite cases (tests/golden/maxima_vjp_composite_cases.json): the chain solve -> feasibility scaling -> solve,
L = sum G . coeffs' + sum w . maxima(coeffs', T'), T' = T max(1, v, sqrt a, cbrt j) of the maxima of coeffs = solve(T),
coeffs' = solve(T').  The solves are tests/golden/gen_vjp_cases.py's dense 60-digit KKT restatement (kkt_solver, imported).
Central differences (step 1e-20) of L in every fixed slot of the fixed values and in every original segment time; every
maximum at a perturbed point is polished by Newton from the unperturbed maximiser.  The limits are drawn so that every
segment's scale is 1 or one active term (v, sqrt a or cbrt j) that leads the next candidate -- 1 included -- and the runner-up
group of its order by at least 5 %, and so that the cases together hold segments of all four kinds; entries whose best and
second-best local maxima are within 1e-3 get w = 0.  One path is ill-conditioned: a 0.05 s segment between 5 s ones.

Run from the repo root:  python3 tests/golden/gen_maxima_vjp_cases.py   (a few minutes)
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from mrs_uav_trajectory_generation_amd import problem as pr  # noqa: E402
from oracle.gen_golden import base, euclid_times, exact_solve, max_magnitude  # noqa: E402

mp.mp.dps = 60
N, D = 10, 4
STEP = mp.mpf("1e-20")
GROUPS = [[0, 1], [2], [3]]
GRID = 800
OUT = os.path.join(ROOT, "tests", "golden", "maxima_vjp_cases.json")
OUT_COMPOSITE = os.path.join(ROOT, "tests", "golden", "maxima_vjp_composite_cases.json")
MARGIN = 1.05


def deriv(c, t, k):
    return sum(base(k, j) * c[j] * t ** (j - k) for j in range(k, N))


def mag2(cs, t, k):
    return sum(deriv(c, t, k) ** 2 for c in cs)


def gfun(cs, t, k):
    """(1/2) d|p^(k)|^2/dt and its derivative"""
    g = sum(deriv(c, t, k) * deriv(c, t, k + 1) for c in cs)
    dg = sum(deriv(c, t, k + 1) ** 2 + deriv(c, t, k) * deriv(c, t, k + 2) for c in cs)
    return g, dg


def newton(cs, t, k, T, iters=8):
    for _ in range(iters):
        g, dg = gfun(cs, t, k)
        if dg == 0:
            break
        t = t - g / dg
    assert 0 <= t <= T
    return t


def local_maxima(cs, T, k):
    """every local maximiser of |p^(k)| on [0, T] (end points included when they are one-sided maxima), 60 digits"""
    T = mp.mpf(T)
    out = []
    g0, _ = gfun(cs, mp.mpf(0), k)
    if g0 < 0 or (g0 == 0 and mag2(cs, mp.mpf(0), k) >= mag2(cs, T / GRID, k)):
        out.append(mp.mpf(0))
    pos_t, pos = mp.mpf(0), g0 > 0   # the last grid point where g was non-zero, and whether it was positive there
    for i in range(1, GRID + 1):
        t = T * i / GRID
        g, _ = gfun(cs, t, k)
        if g == 0:
            continue
        if pos and g < 0:   # + -> - (through exact zeros on grid points): a maximum inside
            lo, hi = pos_t, t
            for _ in range(40):
                mid = (lo + hi) / 2
                if gfun(cs, mid, k)[0] > 0:
                    lo = mid
                else:
                    hi = mid
            out.append(newton(cs, (lo + hi) / 2, k, T))
        pos_t, pos = t, g > 0
    gT, _ = gfun(cs, T, k)
    if gT > 0 or (gT == 0 and mag2(cs, T, k) >= mag2(cs, T * (GRID - 1) / GRID, k)):
        out.append(T)
    return out


def local_value(cs, T, k, t0, at_end):
    """|p^(k)| at the local maximiser near t0 of (cs, T): Newton from t0, or the end point itself"""
    if at_end == 0:
        t = mp.mpf(0)
    elif at_end == 1:
        t = mp.mpf(T)
    else:
        t = newton(cs, t0, k, T, iters=4)
    return mp.sqrt(mag2(cs, t, k))


def entry_gradient(c, T, k, grp, t0):
    """central differences of the local maximum at t0: dM/dc [4][10] and dM/dT"""
    Tm = mp.mpf(T)
    at_end = 0 if t0 == 0 else (1 if t0 == Tm else -1)
    cs = [[mp.mpf(x) for x in c[q]] for q in GROUPS[grp]]
    gc = [[0.0] * N for _ in range(D)]
    for qi, q in enumerate(GROUPS[grp]):
        for j in range(N):
            vals = []
            for sgn in (1, -1):
                cp = [list(x) for x in cs]
                cp[qi][j] += sgn * STEP
                vals.append(local_value(cp, Tm, k, t0, at_end))
            gc[q][j] = float((vals[0] - vals[1]) / (2 * STEP))
    vals = [local_value(cs, Tm + sgn * STEP, k, t0, at_end) for sgn in (1, -1)]
    gT = float((vals[0] - vals[1]) / (2 * STEP))
    return gc, gT


def segment_record(name, c, T):
    c = [[float(x) for x in dim] for dim in c]
    T = float(T)
    entries = []
    for k in (1, 2, 3):
        for grp in range(3):
            cs = [[mp.mpf(x) for x in c[q]] for q in GROUPS[grp]]
            cands = local_maxima(cs, T, k)
            vals = [mp.sqrt(mag2(cs, t, k)) for t in cands]
            M = max(vals) if vals else mp.mpf(0)
            ref = max_magnitude(c, T, k, GROUPS[grp])
            assert abs(M - ref) <= mp.mpf("1e-40") * max(ref, 1), (name, k, grp, M, ref)
            e = dict(k=k, group=grp, maximum=float(M))
            if M == 0:   # a zero maximum: the search keeps its first candidate, t = 0; the rule gives zero gradients
                e.update(t=0.0, grad_coeffs=[[0.0] * N for _ in range(D)], grad_T=0.0, gap=None)
                entries.append(e)
                continue
            order = sorted(range(len(cands)), key=lambda i: -vals[i])
            winners = [i for i in order if vals[order[0]] - vals[i] <= mp.mpf("1e-30") * M]
            second = [vals[i] for i in order if i not in winners]
            e["gap"] = float((M - second[0]) / M) if second else None
            alts = []
            for i in winners:
                gc, gT = entry_gradient(c, T, k, grp, cands[i])
                alts.append(dict(t=float(cands[i]), grad_coeffs=gc, grad_T=gT))
            e.update(alts[0])
            if len(alts) > 1:
                e["alternatives"] = alts
            entries.append(e)
    return dict(name=name, coeffs=c, T=T, entries=entries)


def solved_segments(d, S, seed, take):
    wp, mask, vals = pr.build_vertices(pr.random_box_waypoints(S, seed), d)
    times = euclid_times(np.asarray(wp), pr.DEFAULT_LIMITS)
    coeffs, _, _, _ = exact_solve(mask, vals, [mp.mpf(float(t)) for t in times], d)
    return [("solved_d%d_seed%d_seg%d" % (d, seed, i), [[float(x) for x in dim] for dim in coeffs[i]], float(times[i]))
            for i in take]


# ------------------------------------------------------------------------------------------------------------------------
# composite cases: solve -> scaling -> solve

def winners_of(c_seg, T):
    """per entry of one segment (mpf coefficients): (t0, at_end, M, gap) of the global maximiser"""
    out = []
    for k in (1, 2, 3):
        for grp in range(3):
            cs = [c_seg[q] for q in GROUPS[grp]]
            cands = local_maxima(cs, T, k)
            vals = [mp.sqrt(mag2(cs, t, k)) for t in cands]
            if not vals or max(vals) == 0:
                out.append((mp.mpf(0), 0, mp.mpf(0), None))
                continue
            order = sorted(range(len(cands)), key=lambda i: -vals[i])
            t0, M = cands[order[0]], vals[order[0]]
            gap = float((M - vals[order[1]]) / M) if len(order) > 1 else None
            out.append((t0, 0 if t0 == 0 else (1 if t0 == mp.mpf(T) else -1), M, gap))
    return out


def maxima_near(c_seg, T, win):
    """the 9 maxima of a (perturbed) segment, each polished from its unperturbed maximiser"""
    res = []
    for w, (t0, at_end, M0, _) in enumerate(win):
        k, grp = w // 3 + 1, w % 3
        res.append(mp.mpf(0) if M0 == 0 else local_value([c_seg[q] for q in GROUPS[grp]], T, k, t0, at_end))
    return res


def scale_of(M9, lim):
    """violation_scaling (mrs_tg_device.hpp) and the index of its active term (0: none, 1: v, 2: sqrt a, 3: cbrt j)"""
    viol = [max(M9[3 * k + g] / lim[3 * k + g] for g in range(3)) for k in range(3)]
    terms = [mp.mpf(1), viol[0], mp.sqrt(viol[1]), mp.cbrt(viol[2])]
    i = max(range(4), key=lambda x: terms[x])
    return terms[i], i, terms


def margins_ok(M9, lim, win):
    _, i, terms = scale_of(M9, lim)
    rest = sorted((terms[x] for x in range(4) if x != i), reverse=True)
    if terms[i] < MARGIN * rest[0]:
        return False, i
    if i > 0:
        k = i - 1
        r = sorted(((M9[3 * k + g] / lim[3 * k + g]), g) for g in range(3))
        if r[2][0] < MARGIN * r[1][0]:
            return False, i
        g = r[2][1]
        gap = win[3 * k + g][3]
        if gap is not None and gap < 1e-3:
            return False, i
    return True, i


def composite_record(name, mask, vals, times, d, seed):
    from gen_vjp_cases import kkt_solver
    rng = np.random.default_rng(seed)
    S = len(times)
    tm = [mp.mpf(t) for t in times]
    vm = [[mp.mpf(float(x)) for x in row] for row in np.asarray(vals).reshape(-1, D)]
    solve0 = kkt_solver(mask, tm, d)
    c1, _ = solve0(vm)
    win1 = [winners_of(c1[s], tm[s]) for s in range(S)]
    M1 = [[w[2] for w in win1[s]] for s in range(S)]
    mx = np.array([[float(x) for x in M1[s]] for s in range(S)])
    top = np.where(mx.max(axis=0) > 0, mx.max(axis=0), 1.0)
    best = None
    for _ in range(4000):   # limits: every segment's scale unambiguous, as many kinds of active term as possible
        lim = top * np.exp(rng.uniform(np.log(0.25), np.log(2.5), 9))
        lm = [mp.mpf(float(x)) for x in lim]
        oks = [margins_ok(M1[s], lm, win1[s]) for s in range(S)]
        if all(o for o, _ in oks):
            kinds = len({i for _, i in oks})
            if best is None or kinds > best[0]:
                best = (kinds, lim, [i for _, i in oks])
            if kinds >= min(S, 4):
                break
    assert best is not None, name
    _, lim, kinds = best
    lm = [mp.mpf(float(x)) for x in lim]
    Tp = [tm[s] * scale_of(M1[s], lm)[0] for s in range(S)]
    c2, _ = kkt_solver(mask, Tp, d)(vm)
    win2 = [winners_of(c2[s], Tp[s]) for s in range(S)]
    G = np.round(rng.standard_normal((S, D, N)) * 64) / 64
    w = np.round(rng.standard_normal((S, 9)) * 64) / 64
    for s in range(S):
        for e in range(9):
            gap = win2[s][e][3]
            if gap is not None and gap < 1e-3:
                w[s, e] = 0.0
    Gm = [[[mp.mpf(float(x)) for x in row] for row in seg] for seg in G]
    wm = [[mp.mpf(float(x)) for x in row] for row in w]

    def L_at(t, v):
        sol = solve0 if t is tm else kkt_solver(mask, t, d)
        ca, _ = sol(v)
        tp = [t[s] * scale_of(maxima_near(ca[s], t[s], win1[s]), lm)[0] for s in range(S)]
        cb, _ = kkt_solver(mask, tp, d)(v)
        L = mp.mpf(0)
        for s in range(S):
            for q in range(D):
                for j in range(N):
                    L += Gm[s][q][j] * cb[s][q][j]
            for e, m in enumerate(maxima_near(cb[s], tp[s], win2[s])):
                L += wm[s][e] * m
        return L

    flat = np.asarray(mask).reshape(-1)
    gv = np.zeros((len(flat), D))
    for i in range(len(flat)):
        if not flat[i]:
            continue
        for q in range(D):
            vals_pm = []
            for sgn in (1, -1):
                v2 = [list(r) for r in vm]
                v2[i][q] += sgn * STEP
                vals_pm.append(L_at(tm, v2))
            gv[i, q] = float((vals_pm[0] - vals_pm[1]) / (2 * STEP))
    gt = np.zeros(S)
    for s in range(S):
        vals_pm = []
        for sgn in (1, -1):
            t2 = list(tm)
            t2[s] = t2[s] + sgn * STEP
            vals_pm.append(L_at(t2, vm))
        gt[s] = float((vals_pm[0] - vals_pm[1]) / (2 * STEP))
    return dict(name=name, derivative_to_optimize=d, fixed_mask=np.asarray(mask).astype(int).tolist(),
                fixed_values=np.asarray(vals).tolist(), seg_times=[float(t) for t in times], limits=[float(x) for x in lim],
                active=kinds, scaled_times=[float(t) for t in Tp], G=G.tolist(), w=w.reshape(S, 3, 3).tolist(),
                grad_fixed_values=gv.reshape(-1, 5, D).tolist(), grad_seg_times=gt.tolist())


def composite_cases():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    out = []
    for name, S, seed, d, times in (("composite_d4_s3", 3, 81, 4, None), ("composite_d3_s4", 4, 82, 3, None),
                                    ("composite_d2_s3", 3, 83, 2, None), ("composite_ill_short_segment", 3, 84, 4, [5.0, 0.05, 5.0])):
        wp, mask, vals = pr.build_vertices(pr.random_box_waypoints(S, seed), d)
        if times is None:
            times = [float(t) for t in euclid_times(np.asarray(wp), pr.DEFAULT_LIMITS)]
        out.append(composite_record(name, mask, vals, times, d, seed))
        print(name, "done, active terms", out[-1]["active"], flush=True)
    kinds = {i for c in out for i in c["active"]}
    assert kinds == {0, 1, 2, 3}, kinds
    with open(OUT_COMPOSITE, "w") as f:
        json.dump(dict(generator="tests/golden/gen_maxima_vjp_cases.py", mp_dps=mp.mp.dps, step="1e-20", cases=out), f)
    print(OUT_COMPOSITE, os.path.getsize(OUT_COMPOSITE), "bytes")


def main():
    if "--composite-only" in sys.argv:
        composite_cases()
        return
    segs = []
    for d, seed in ((2, 71), (3, 72), (4, 73)):
        segs += solved_segments(d, 4, seed, (0, 2))
    z = [0.0] * N
    # end point: |v|, |a|, |j| of {x, y} grow on [0, 1.5]; the heading is constant (zero maxima)
    segs.append(("end_point_maximum", [[0.5, 0.0, 1.0, 0.1, 0.02] + [0.0] * 5, [0.0, 0.25] + [0.0] * 8,
                                       [1.0, -0.5, 0.0, 0.05, 0.01] + [0.0] * 5, [0.3] + [0.0] * 9], 1.5))
    # start point: |v| of {x, y} and |v|, |a| of the heading are largest at t = 0
    segs.append(("start_point_maximum", [[0.0, 2.0, -0.5, 0.1, 0.05] + [0.0] * 5, [1.0, -1.0, 0.25, -0.05, 0.02] + [0.0] * 5,
                                         list(z), [0.0, 0.8, -0.3, 0.02, 0.01] + [0.0] * 5], 1.0))
    # constant heading (zero maxima) on a solved segment
    name, c, T = solved_segments(4, 4, 74, (1,))[0]
    c[3] = [c[3][0]] + [0.0] * 9
    segs.append(("constant_heading", c, T))
    # rest to rest 0 -> 1 along z over T = 2: 35 s^4 - 84 s^5 + 70 s^6 - 20 s^7, s = t / 2 (exact in double); the
    # acceleration is odd about t = 1, so its two peaks tie
    rr = [0.0] * N
    for j, a in ((4, 35.0), (5, -84.0), (6, 70.0), (7, -20.0)):
        rr[j] = a / 2.0 ** j
    segs.append(("rest_to_rest_tie", [[0.2, 0.1, 0.05, 0.01, 0.002] + [0.0] * 5, [0.0] * N, rr, [0.0] * N], 2.0))
    cases = []
    for name, c, T in segs:
        cases.append(segment_record(name, c, T))
        print(name, "done", flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(generator="tests/golden/gen_maxima_vjp_cases.py", mp_dps=mp.mp.dps, step="1e-20", cases=cases), f)
    print(OUT, os.path.getsize(OUT), "bytes")
    composite_cases()


if __name__ == "__main__":
    main()

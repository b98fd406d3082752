#!/usr/bin/env python3
"""Generate tests/golden/deviation_cases.json: 60-digit gradients of a loss on the deviations of a sampled trajectory from its
waypoint polyline, for mrs_tg_plan_path_deviation_vjp (csrc/mrs_tg_deviation.hpp).

The ground truth is NOT the table of the header: it is central differences (step 1e-20) of L = sum_i g_i d_i over an
exact-arithmetic restatement of distFromSegment, in every coordinate of every scanned sample and of every waypoint, WITH THE
CURSORS HELD FIXED at what the double-precision scan finds (restated here in Python floats, which are IEEE doubles with
nothing fused).  Upstreams are dyadic, so they are exact in double; samples and waypoints are taken as exact doubles.

The generator asserts that every differentiated sample keeps the margins |coord| >= 1e-6 len, |coord - len| >= 1e-6 len and
d >= 1e-3: inside them the branch cannot change within the step, and the exact branch is the double scan's.

Tie cases ("tie": true) have exactly representable coordinates and sit ON the kinks: coord == 0, coord == len, coincident
waypoints (len == 0), a sample on its segment (d == 0), a zero upstream.  They are exempt from the margins; their gradients are
the closed form of the branch the forward takes -- the end rows (p - a)/d or (p - b)/d, the interior row u = e/d split
-(1 - tau) u / -tau u with tau = coord/len (0 when len == 0), exactly 0 for d == 0 -- evaluated at 60 digits.

Run from the repo root:  python3 tests/golden/gen_deviation_cases.py   (some seconds)
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from tests import deviation_util as du  # noqa: E402

mp.mp.dps = 60
STEP = mp.mpf("1e-20")
OUT = os.path.join(ROOT, "tests", "golden", "deviation_cases.json")


def double_dist(p, a, b):
    """distFromSegment in doubles, operation by operation: (d, branch, coord, len); branch -1: coord < 0, +1: coord > len"""
    sv = [b[k] - a[k] for k in range(3)]
    ln = float(np.sqrt(sv[0] * sv[0] + sv[1] * sv[1] + sv[2] * sv[2]))
    n = list(sv)
    if ln * ln > 0:
        n = [v / ln for v in sv]
    d1 = [p[k] - a[k] for k in range(3)]
    coord = n[0] * d1[0] + n[1] * d1[1] + n[2] * d1[2]
    if coord < 0:
        return float(np.sqrt(d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2])), -1, coord, ln
    if coord > ln:
        e = [p[k] - b[k] for k in range(3)]
        return float(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])), 1, coord, ln
    f = [p[k] - (a[k] + n[k] * coord) for k in range(3)]
    return float(np.sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2])), 0, coord, ln


def double_scan(w, s):
    """(cursor, branch, coord, len, d) per scanned sample, by the rule in doubles"""
    S, c, rows = len(w) - 1, 0, []
    for i in range(len(s) - 1):
        d, br, coord, ln = double_dist(s[i], w[c], w[c + 1])
        rows.append((c, br, coord, ln, d))
        if double_dist(w[c + 1], s[i], s[i + 1])[0] < du.ADVANCE and c < S - 1:
            c += 1
    return rows


def norm(v):
    return mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def exact_dist(p, a, b):
    sv = [b[k] - a[k] for k in range(3)]
    ln = norm(sv)
    n = [v / ln for v in sv] if ln > 0 else sv
    d1 = [p[k] - a[k] for k in range(3)]
    coord = sum(n[k] * d1[k] for k in range(3))
    if coord < 0:
        return norm(d1), -1
    if coord > ln:
        return norm([p[k] - b[k] for k in range(3)]), 1
    return norm([p[k] - (a[k] + n[k] * coord) for k in range(3)]), 0


def closed_form(p, a, b, branch):
    """(dd/dp, dd/da, dd/db) of the given branch at 60 digits; zeros for d == 0"""
    zero = [mp.mpf(0)] * 3
    if branch < 0:
        r = [p[k] - a[k] for k in range(3)]
        d = norm(r)
        if d == 0:
            return zero, zero, zero
        u = [v / d for v in r]
        return u, [-v for v in u], zero
    if branch > 0:
        r = [p[k] - b[k] for k in range(3)]
        d = norm(r)
        if d == 0:
            return zero, zero, zero
        u = [v / d for v in r]
        return u, zero, [-v for v in u]
    sv = [b[k] - a[k] for k in range(3)]
    ln = norm(sv)
    n = [v / ln for v in sv] if ln > 0 else sv
    coord = sum(n[k] * (p[k] - a[k]) for k in range(3))
    e = [p[k] - (a[k] + n[k] * coord) for k in range(3)]
    d = norm(e)
    if d == 0:
        return zero, zero, zero
    tau = coord / ln if ln > 0 else mp.mpf(0)
    u = [v / d for v in e]
    return u, [-(1 - tau) * v for v in u], [-tau * v for v in u]


def make_case(name, w, s, g, tie=False, first_segment=1):
    w = [[float(x) for x in row[:3]] for row in w]
    s = [[float(x) for x in row[:3]] for row in s]
    g = [float(x) for x in g]
    rows = double_scan(w, s)
    k = len(rows)
    assert len(g) == k
    W = [[mp.mpf(x) for x in row] for row in w]
    P = [[mp.mpf(x) for x in row] for row in s]
    G = [mp.mpf(x) for x in g]
    gs = [[mp.mpf(0)] * 3 for _ in range(k)]
    gw = [[mp.mpf(0)] * 3 for _ in range(len(w))]
    for i, (c, br, coord, ln, d) in enumerate(rows):
        if tie:
            dp, da, db = closed_form(P[i], W[c], W[c + 1], br)
            for j in range(3):
                gs[i][j] = G[i] * dp[j]
                gw[c][j] += G[i] * da[j]
                gw[c + 1][j] += G[i] * db[j]
            continue
        assert abs(coord) >= 1e-6 * ln and abs(coord - ln) >= 1e-6 * ln and d >= 1e-3, (name, i, coord, ln, d)
        assert exact_dist(P[i], W[c], W[c + 1])[1] == br, (name, i)

        def moved(what, j, h, i=i, c=c):
            p, a, b = list(P[i]), list(W[c]), list(W[c + 1])
            {"p": p, "a": a, "b": b}[what][j] += h
            val, branch = exact_dist(p, a, b)
            assert branch == rows[i][1]
            return val

        for j in range(3):
            gs[i][j] = G[i] * (moved("p", j, STEP) - moved("p", j, -STEP)) / (2 * STEP)
            gw[c][j] += G[i] * (moved("a", j, STEP) - moved("a", j, -STEP)) / (2 * STEP)
            gw[c + 1][j] += G[i] * (moved("b", j, STEP) - moved("b", j, -STEP)) / (2 * STEP)
    f = lambda x: float(mp.nstr(x, 17))   # noqa: E731
    return dict(name=name, tie=bool(tie), first_segment=first_segment, waypoints=w, samples=s, upstream=g,
                cursor=[r[0] for r in rows], branch=[r[1] for r in rows], grad_samples=[[f(x) for x in row] for row in gs],
                grad_waypoints=[[f(x) for x in row] for row in gw])


def offset_walk(w, n, amplitude, seed, through=True, lead=0):
    """du.walk with a bump that never vanishes (0.1 of the amplitude at the waypoints and flat there: near enough for the cursor to follow,
    far enough for d >= 1e-3); lead: samples in front of w_0, on the first segment's line produced backwards (coord < 0)"""
    rng = np.random.default_rng(seed)
    w = np.asarray(w, dtype=np.float64)
    seg = np.linalg.norm(np.diff(w, axis=0), axis=1)
    cum = np.concatenate([[0.0], np.cumsum(seg)])
    side = rng.standard_normal((len(seg), 3))
    side /= np.linalg.norm(side, axis=1)[:, None]
    out = []
    for i in range(-lead, n):
        a = cum[-1] * i / (n - 1)
        j = min(max(int(np.searchsorted(cum, a, side="right")) - 1, 0), len(seg) - 1)
        f = (a - cum[j]) / seg[j]
        bump = 0.1 + 0.9 * np.sin(np.pi * min(max(f, 0.0), 1.0)) ** 2 if through else 1.0
        out.append(w[j] + f * (w[j + 1] - w[j]) + amplitude * bump * side[j])
    return np.array(out)


def main():
    rng = np.random.default_rng(11)
    cases = []

    def add(name, w, s, **kw):
        cases.append(make_case(name, w, s, du.dyadic(rng, len(s) - 1), **kw))
        c = cases[-1]
        print("%-28s S %2d  scanned %3d  cursors up to %d  branches %s" % (name, len(c["waypoints"]) - 1, len(c["cursor"]),
                                                                           max(c["cursor"]), sorted(set(c["branch"]))))

    w = du.polyline(1, 21)
    add("one_segment", w, offset_walk(w, 20, 0.15, 1))
    w = du.polyline(3, 22, 0.5, 0.9)
    add("three_segments", w, offset_walk(w, 60, 0.12, 2))
    assert max(cases[-1]["cursor"]) == 2
    w = du.polyline(10, 23, 0.5, 0.9)
    add("ten_segments_two_chunks", w, offset_walk(w, 150, 0.1, 3))
    assert max(cases[-1]["cursor"]) == 9 and len(cases[-1]["cursor"]) > 128
    w = du.polyline(3, 24)
    add("cursor_sticks", w, offset_walk(w, 50, 0.2, 4, through=False))
    w = du.polyline(2, 25, 0.5, 0.9)
    add("starts_behind_w0", w, offset_walk(w, 40, 0.1, 5, lead=4), first_segment=0)
    assert max(cases[-1]["cursor"]) == 1
    # ties: dyadic coordinates, an axis-parallel polyline whose second and third waypoint coincide
    w = [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 3.0, 0.0]]
    s = [[0.0, 0.5, 0.0],      # coord == 0: the interior row
         [0.5, 0.0, 0.0],      # on the segment: d == 0
         [1.0, 0.25, 0.25],
         [1.75, 0.25, 0.0],
         [2.0, 0.0625, 0.0],   # coord == len: the interior row; the step to the next sample passes w_1: the cursor moves on
         [2.0, -0.03125, 0.03125],   # segment 1 has no length: everything goes to a; the step passes w_2
         [2.0, 0.5, 0.25],       # segment 2
         [2.0, 1.0, 0.0],        # on the segment
         [2.0, 3.0, 0.5],        # coord == len
         [2.25, 3.5, 0.0],       # behind the end
         [2.0, 4.0, 0.0]]
    c = make_case("tie_exact_coordinates", w, s, [1.0, 0.5, -0.75, 0.0, 1.25, -1.0, 0.5, 2.0, -0.5, 1.5], tie=True)
    assert c["cursor"] == [0, 0, 0, 0, 0, 1, 2, 2, 2, 2] and c["branch"] == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1], (c["cursor"], c["branch"])
    cases.append(c)
    with open(OUT, "w") as f:
        json.dump(dict(step="1e-20", digits=60, cases=cases), f, separators=(",", ":"))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()

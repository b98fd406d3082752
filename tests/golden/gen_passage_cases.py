#!/usr/bin/env python3
"""Generate tests/golden/passage_cases.json: 60-digit gradients of a loss on the miss distances and on the foot-point
fractions of the waypoints a sampled trajectory passes, for mrs_tg_plan_waypoint_passage_vjp (csrc/mrs_tg_passage.hpp,
DESIGN.md section 11c).

The ground truth is NOT the table of the header: it is central differences (step 1e-20) of L_m = sum_k g_k m_k and of
L_t = sum_k h_k tau_k over an exact-arithmetic restatement of distFromSegment and of tau, in every coordinate of every sample
and of every waypoint, WITH THE INDICES HELD FIXED at what the double-precision scan finds (restated here in Python floats,
which are IEEE doubles with nothing fused).  The two losses are differentiated apart, so that each of the two derived bounds
is tested on its own rows.  Upstreams are dyadic, so they are exact in double; samples and waypoints are taken as exact doubles.

The generator asserts that every hit keeps the margins |coord| >= 1e-6 len, |coord - len| >= 1e-6 len, len >= 0.05 and
1e-4 <= m <= 0.099: inside them neither the branch nor the hit can change within the step.

Run from the repo root:  python3 tests/golden/gen_passage_cases.py   (some seconds)
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from tests import deviation_util as du  # noqa: E402
from tests import passage_util as pu  # noqa: E402
from tests.golden.gen_deviation_cases import double_dist, norm  # noqa: E402

mp.mp.dps = 60
STEP = mp.mpf("1e-20")
OUT = os.path.join(ROOT, "tests", "golden", "passage_cases.json")


def double_scan(w, s):
    """(index, branch, coord, len, m) per waypoint reached, by the rule in doubles"""
    c, hits = 0, []
    for i in range(len(s) - 1):
        if c == len(w):
            break
        m, br, coord, ln = double_dist(w[c], s[i], s[i + 1])
        if m < pu.PASS:
            hits.append((i, br, coord, ln, m))
            c += 1
    return hits


def exact(p, a, b):
    """(m, tau, branch) of p against the step a -> b in exact arithmetic"""
    sv = [b[k] - a[k] for k in range(3)]
    ln = norm(sv)
    n = [v / ln for v in sv]
    q = [p[k] - a[k] for k in range(3)]
    coord = sum(n[k] * q[k] for k in range(3))
    if coord < 0:
        return norm(q), mp.mpf(0), -1
    if coord > ln:
        return norm([p[k] - b[k] for k in range(3)]), mp.mpf(1), 1
    return norm([p[k] - (a[k] + n[k] * coord) for k in range(3)]), coord / ln, 0


def make_case(name, w, s, gm, gt):
    w = [[float(x) for x in row[:3]] for row in w]
    s = [[float(x) for x in row[:3]] for row in s]
    hits = double_scan(w, s)
    W, P = [[mp.mpf(x) for x in row] for row in w], [[mp.mpf(x) for x in row] for row in s]
    zeros = lambda n: [[mp.mpf(0)] * 3 for _ in range(n)]   # noqa: E731
    out = {}
    for which, g in ((0, gm), (1, gt)):
        gs, gw = zeros(len(s)), zeros(len(w))
        for k, (i, br, coord, ln, m) in enumerate(hits):
            assert abs(coord) >= 1e-6 * ln and abs(coord - ln) >= 1e-6 * ln and ln >= 0.05 and 1e-4 <= m <= 0.099, (name, k, coord, ln, m)
            assert exact(W[k], P[i], P[i + 1])[2] == br, (name, k)

            def moved(what, j, h, k=k, i=i, br=br):
                p, a, b = list(W[k]), list(P[i]), list(P[i + 1])
                {"p": p, "a": a, "b": b}[what][j] += h
                val = exact(p, a, b)
                assert val[2] == br
                return val[which]

            G = mp.mpf(float(g[k]))
            for j in range(3):
                gw[k][j] += G * (moved("p", j, STEP) - moved("p", j, -STEP)) / (2 * STEP)
                gs[i][j] += G * (moved("a", j, STEP) - moved("a", j, -STEP)) / (2 * STEP)
                gs[i + 1][j] += G * (moved("b", j, STEP) - moved("b", j, -STEP)) / (2 * STEP)
        f = lambda x: float(mp.nstr(x, 17))   # noqa: E731
        tag = "miss" if which == 0 else "fraction"
        out["grad_samples_" + tag] = [[f(x) for x in row] for row in gs]
        out["grad_waypoints_" + tag] = [[f(x) for x in row] for row in gw]
    return dict(name=name, waypoints=w, samples=s, grad_miss=[float(x) for x in gm], grad_fraction=[float(x) for x in gt],
                index=[h[0] for h in hits], branch=[h[1] for h in hits], **out)


def main():
    rng = np.random.default_rng(12)
    cases = []

    def add(name, w, s):
        cases.append(make_case(name, w, s, du.dyadic(rng, len(w)), du.dyadic(rng, len(w))))
        c = cases[-1]
        print("%-28s W %2d  samples %3d  reached %2d  branches %s" % (name, len(w), len(s), len(c["index"]), sorted(set(c["branch"]))))

    def jitter(s, amount):
        return s + rng.uniform(-amount, amount, s.shape)

    s = jitter(pu.straight(40, z=0.5), 0.02)
    add("five_beside_their_steps", [np.array(pu.on_step(4 + 7 * j, 0.0, z=0.5)) + rng.uniform(0.01, 0.04, 3) * [0, 1, 1] for j in range(5)], s)
    assert cases[-1]["index"] == [4, 11, 18, 25, 32] and set(cases[-1]["branch"]) == {0}
    # behind a step's end (coord > len) and, on the step after a hit, in front of a step's start (coord < 0)
    s = jitter(pu.straight(30), 0.01)
    w = [s[6] + [0.03, 0.02, 0.01],          # 0.03 behind the end of step 5: taken by step 5
         s[12] + [-0.1, 0.03, 0.0],          # beside step 11
         s[12] + [-0.04, -0.03, 0.02],       # in front of the start of step 12, tested by it first: coord < 0
         s[20] + [0.125, 0.0, 0.05]]
    add("both_end_branches", w, s)
    assert cases[-1]["index"] == [5, 11, 12, 20] and cases[-1]["branch"] == [1, 0, -1, 0], (cases[-1]["index"], cases[-1]["branch"])
    # hits on steps 63 and 64: sample row 64 takes a b-part and an a-part
    s = jitter(pu.straight(70, z=-0.25), 0.015)
    add("across_the_seam", [pu.on_step(30, 0.03, z=-0.25), pu.on_step(63, 0.04, z=-0.22), pu.on_step(64, -0.03, z=-0.27)], s)
    assert cases[-1]["index"] == [30, 63, 64]
    # a curved walk in three dimensions with short steps (len 0.05 .. 0.1) far from the origin
    w = du.polyline(4, 31, 0.6, 0.9) + [40.0, -25.0, 12.0]
    s = du.walk(w, 45, 0.0, 1)
    add("far_from_the_origin", w + rng.uniform(0.005, 0.02, w.shape), s)
    assert len(cases[-1]["index"]) == 5
    s = jitter(pu.straight(40, z=0.5), 0.02) + [40.0, -25.0, 12.0]
    add("far_from_the_origin_beside", [s[4 + 7 * j] + [0.1, 0.0, 0.0] + rng.uniform(0.01, 0.04, 3) * [0, 1, 1] for j in range(5)], s)
    assert cases[-1]["index"] == [4, 11, 18, 25, 32] and set(cases[-1]["branch"]) == {0}
    with open(OUT, "w") as f:
        json.dump(dict(step="1e-20", digits=60, cases=cases), f, separators=(",", ":"))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()

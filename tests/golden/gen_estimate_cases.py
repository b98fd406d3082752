#!/usr/bin/env python3
"""Generate tests/golden/estimate_cases.json: 60-digit values and gradients of the Euclidean segment-time estimate, for
mrs_tg_plan_estimate_times_vjp (csrc/mrs_tg_estimate_vjp.hpp).

The ground truth is NOT the table of the header: it is central differences (step 1e-20) of L = sum_i g_i t_i over an
exact-arithmetic restatement of estimateSegmentTimesEuclidean AS THE REFERENCE WRITES IT -- atan2, the distance over
v_v / sin or v_h / cos of the inclination, the floor, the wrapped heading difference, 1.5 (t_vel + t_acc) -- in every waypoint
coordinate and in limits 0, 1, 2 and 5, with every branch decided by the exact values.  Waypoints, limits and upstreams are
taken as exact doubles; upstreams are dyadic.  The header's closed forms are evaluated at 60 digits beside it only to (a) assert
that the two agree to 1e-30 and (b) record, per output entry, the sum of the absolute values of its contributions, taken at
the granularity at which the kernel rounds: one contribution per segment for a waypoint entry and for v_h and v_v, and the
addends of the heading term one by one -- 1.5 |g| (ang/w^2, 1/a when cruising, 2/a when accelerating) for w, 1.5 |g| (w/a^2
when cruising, 2 w/a^2 when accelerating) for a -- because those cancel inside one segment.

Margins.  Every segment stays at least 1e-3 away from every branch boundary -- |inclination| against atan2(v_v, v_h), the
distance term against 0.01, the heading term against the distance term, `reduced` against 0, ang against pi/4 -- except where
the boundary is the point of the case ("boundary" names it): coincident waypoints (distance 0, inclination atan2(0, 0)), the
+-pi seam (the heading difference wraps), equal headings (delta = 0).  The generator asserts the margins and that the term of
the double-precision forward (restated here in Python floats) is the exact one.

Run from the repo root:  python3 tests/golden/gen_estimate_cases.py   (some seconds)
"""
import json
import math
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from tests import estimate_util as eu  # noqa: E402

mp.mp.dps = 60
STEP = mp.mpf("1e-20")
MARGIN = 1e-3
OUT = eu.FIXTURES
FLT_MAX = eu.FLT_MAX
DEFAULT = [2.0, 2.0, 1.0, 2.0, 2.0, 2.0, 20.0, 20.0, 20.0]


def exact_delta(a, b):
    """the heading difference start minus end brought into [-pi, pi) with the exact pi"""
    two_pi = 2 * mp.pi
    d = (a - b + mp.pi) % two_pi    # mpmath's % takes the sign of the divisor: [0, 2 pi)
    return d - mp.pi


def exact_segment(s, e, lim):
    """-> dict(t, term, cruise, acc, margins...) of one segment, every quantity an mpf"""
    v_h, v_v, w, a = lim[0], lim[1], lim[2], lim[5]
    dx, dy, dz = e[0] - s[0], e[1] - s[1], e[2] - s[2]
    h = mp.sqrt(dx * dx + dy * dy)
    incl = mp.atan2(dz, h)
    thr = mp.atan2(v_v, v_h)
    vertical = incl > thr or incl < -thr
    vmax = abs(v_v / mp.sin(incl)) if vertical else abs(v_h / mp.cos(incl))
    t_dist = mp.sqrt(dx * dx + dy * dy + dz * dz) / vmax
    floored = t_dist < mp.mpf("0.01")
    t = mp.mpf("0.01") if floored else t_dist
    delta = exact_delta(s[3], e[3])
    ang = abs(delta)
    cruise = acc = False
    t_vel = t_acc = mp.mpf(0)
    relaxed = not (w < FLT_MAX and a < FLT_MAX)
    reduced = None
    if not relaxed:
        reduced = (ang - w * w / a) / w
        cruise = not reduced < 0
        t_vel = ang / w if reduced < 0 else reduced
        if ang > mp.pi / 4:
            acc = True
            t_acc = 2 * (w / a)
    hf = mp.mpf("1.5") * (t_vel + t_acc)
    heading = hf > t
    term = eu.HEADING if heading else eu.FLOOR if floored else eu.VERTICAL if vertical else eu.HORIZONTAL
    return dict(t=hf if heading else t, term=term, cruise=cruise, acc=acc, relaxed=relaxed, incl=incl, thr=thr, t_dist=t_dist,
                hf=hf, reduced=reduced, ang=ang, delta=delta, h=h, dx=dx, dy=dy, dz=dz)


def double_term(s, e, lim):
    """the forward in Python floats (IEEE doubles, nothing fused), operation by operation -> (term, value)"""
    v_h, v_v, w, a = lim[0], lim[1], lim[2], lim[5]
    dx, dy, dz = e[0] - s[0], e[1] - s[1], e[2] - s[2]
    incl = math.atan2(dz, math.sqrt(dx * dx + dy * dy))
    thr = math.atan2(v_v, v_h)
    vertical = incl > thr or incl < -thr
    vmax = abs(v_v / math.sin(incl)) if vertical else abs(v_h / math.cos(incl))
    t = math.sqrt(dx * dx + dy * dy + dz * dz) / vmax
    floored = t < 0.01
    if floored:
        t = 0.01

    def wrap(x):
        r = math.fmod(x + math.pi, 2.0 * math.pi)
        if r < 0:
            r += 2.0 * math.pi
        return r - math.pi
    d = wrap(s[3]) - wrap(e[3])
    if d < -math.pi:
        d += 2.0 * math.pi
    elif d >= math.pi:
        d -= 2.0 * math.pi
    ang = abs(d)
    t_vel = t_acc = 0.0
    if w < FLT_MAX and a < FLT_MAX:
        reduced = (ang - (w * w) / a) / w
        t_vel = ang / w if reduced < 0 else reduced
        if ang > math.pi / 4:
            t_acc = 2 * (w / a)
    hf = 1.5 * (t_vel + t_acc)
    if hf > t:
        return eu.HEADING, hf
    return (eu.FLOOR if floored else eu.VERTICAL if vertical else eu.HORIZONTAL), t


def closed_form(x, lim, g):
    """the header's table at 60 digits -> (d/de [4], d/dlimits {index: value}, |addends| per limit index), times g"""
    de, dl, sl = [mp.mpf(0)] * 4, {}, {}
    v_h, v_v, w, a = lim[0], lim[1], lim[2], lim[5]
    sign = lambda v: mp.mpf(1 if v > 0 else -1 if v < 0 else 0)   # noqa: E731
    if x["term"] == eu.HORIZONTAL:
        de[0], de[1] = g * x["dx"] / x["h"] / v_h, g * x["dy"] / x["h"] / v_h
        dl[0] = -g * x["h"] / v_h / v_h
        sl[0] = abs(dl[0])
    elif x["term"] == eu.VERTICAL:
        de[2] = g * sign(x["dz"]) / v_v
        dl[1] = -g * abs(x["dz"]) / v_v / v_v
        sl[1] = abs(dl[1])
    elif x["term"] == eu.HEADING:
        de[3] = -g * mp.mpf("1.5") * sign(x["delta"]) / w
        parts_w = [-x["ang"] / (w * w)] + ([-1 / a] if x["cruise"] else []) + ([2 / a] if x["acc"] else [])
        parts_a = ([w / (a * a)] if x["cruise"] else []) + ([-2 * w / (a * a)] if x["acc"] else [])
        dl[2], dl[5] = g * mp.mpf("1.5") * sum(parts_w), g * mp.mpf("1.5") * sum(parts_a)
        sl[2] = abs(g) * mp.mpf("1.5") * sum(abs(v) for v in parts_w)
        sl[5] = abs(g) * mp.mpf("1.5") * sum(abs(v) for v in parts_a)
    return de, dl, sl


def check_margins(name, j, x, boundary):
    def away(v, what):
        assert abs(v) >= MARGIN, (name, j, what, float(v))
    if "coincident" not in boundary:
        away(abs(x["incl"]) - x["thr"], "inclination against atan2(v_v, v_h)")
    away(x["t_dist"] - mp.mpf("0.01"), "distance term against the floor")
    away(x["hf"] - max(x["t_dist"], mp.mpf("0.01")), "heading term against the distance term")
    if not x["relaxed"]:
        away(x["reduced"], "reduced against 0")
        away(x["ang"] - mp.pi / 4, "ang against pi/4")
    if "seam" not in boundary:
        away(mp.pi - x["ang"], "heading difference against the seam")
    if "equal_headings" not in boundary:
        away(x["ang"], "heading difference against 0")


def make_case(name, waypoints, limits, upstream, boundary=()):
    w = [[mp.mpf(float(v)) for v in row] for row in waypoints]
    lim = [mp.mpf(float(v)) for v in limits]
    g = [mp.mpf(float(v)) for v in upstream]
    S = len(w) - 1
    assert len(g) == S and all(float(v) * 64 == round(float(v) * 64) for v in upstream)
    segs = [exact_segment(w[j], w[j + 1], lim) for j in range(S)]
    for j, x in enumerate(segs):
        check_margins(name, j, x, boundary)
        term, value = double_term([float(v) for v in waypoints[j]], [float(v) for v in waypoints[j + 1]], [float(v) for v in limits])
        assert term == x["term"], (name, j, term, x["term"])
        assert abs(value - x["t"]) <= 1e-13 * x["t"], (name, j)

    def loss(wq, lq):
        total = mp.mpf(0)
        for j in range(S):
            y = exact_segment(wq[j], wq[j + 1], lq)
            assert y["term"] == segs[j]["term"] and y["cruise"] == segs[j]["cruise"] and y["acc"] == segs[j]["acc"], (name, j)
            total += g[j] * y["t"]
        return total

    gw = [[mp.mpf(0)] * 4 for _ in range(S + 1)]
    for v in range(S + 1):
        for k in range(4):
            up = [list(r) for r in w]
            dn = [list(r) for r in w]
            up[v][k] += STEP
            dn[v][k] -= STEP
            gw[v][k] = (loss(up, lim) - loss(dn, lim)) / (2 * STEP)
    gl = [mp.mpf(0)] * 9
    for k in eu.READ_LIMITS:
        if lim[k] >= FLT_MAX:
            continue   # (a relaxed limit: the estimate does not depend on it)
        up, dn = list(lim), list(lim)
        up[k] += STEP
        dn[k] -= STEP
        gl[k] = (loss(w, up) - loss(w, dn)) / (2 * STEP)
    # the header's table: agreement, and the sums of |contributions|
    cw = [[mp.mpf(0)] * 4 for _ in range(S + 1)]
    sw = [[mp.mpf(0)] * 4 for _ in range(S + 1)]
    cl, sl = [mp.mpf(0)] * 9, [mp.mpf(0)] * 9
    for j, x in enumerate(segs):
        de, dl, sla = closed_form(x, lim, g[j])
        for k in range(4):
            cw[j + 1][k] += de[k]
            cw[j][k] -= de[k]
            sw[j + 1][k] += abs(de[k])
            sw[j][k] += abs(de[k])
        for k, v in dl.items():
            cl[k] += v
            sl[k] += sla[k]
    for v in range(S + 1):
        for k in range(4):
            assert abs(cw[v][k] - gw[v][k]) <= mp.mpf("1e-30") * (1 + sw[v][k]), (name, v, k, cw[v][k], gw[v][k])
    for k in range(9):
        assert abs(cl[k] - gl[k]) <= mp.mpf("1e-30") * (1 + sl[k]), (name, k, cl[k], gl[k])
    f = lambda v: float(v)   # noqa: E731
    return dict(name=name, boundary=list(boundary), waypoints=[[float(v) for v in r] for r in waypoints],
                limits=[float(v) for v in limits], upstream=[float(v) for v in upstream], term=[x["term"] for x in segs],
                cruise=[bool(x["cruise"]) for x in segs], acc=[bool(x["acc"]) for x in segs], value=[f(x["t"]) for x in segs],
                grad_waypoints=[[f(v) for v in r] for r in gw], grad_limits=[f(v) for v in gl],
                scale_waypoints=[[f(v) for v in r] for r in sw], scale_limits=[f(v) for v in sl])


def limits_with(**kw):
    lim = list(DEFAULT)
    for k, v in kw.items():
        lim[dict(v_h=0, v_v=1, w=2, a=5)[k]] = v
    return lim


def random_path(seed, S):
    """box-like waypoints with limits drawn from [0.3, 4], re-drawn until every segment keeps the margins"""
    for attempt in range(200):
        rng = np.random.default_rng(seed * 1000 + attempt)
        w = np.column_stack([rng.uniform(-4, 4, S + 1), rng.uniform(-4, 4, S + 1), rng.uniform(1, 6, S + 1),
                             np.cumsum(rng.uniform(-1.6, 1.6, S + 1))])
        lim = rng.uniform(0.3, 4.0, 9)
        try:
            return make_case("limits_drawn_%d" % seed, w, lim, eu.dyadic(rng, S))
        except AssertionError:
            continue
    raise RuntimeError("no draw kept the margins")


def main():
    cases = [
        make_case("horizontal", [[0, 0, 5, 0], [3, 4, 5.5, 0.2]], DEFAULT, [0.75]),
        make_case("vertical_climb", [[0, 0, 1, 0], [1, 0.5, 4, 0.1]], DEFAULT, [-0.5]),
        make_case("vertical_descent", [[0.25, 0, 7, 0.3], [1, 0.5, 2.5, 0.2]], limits_with(v_v=1.0), [0.625]),
        make_case("exactly_flat", [[1, 2, 5, 0.3], [4, -2, 5, 0.1]], DEFAULT, [1.0]),
        make_case("purely_vertical", [[1, 1, 2, 0.1], [1, 1, 5, 0.2]], DEFAULT, [-0.25]),
        make_case("coincident_waypoints", [[1, 1, 1, 0.5], [1, 1, 1, 0.5]], DEFAULT, [0.5],
                  boundary=("coincident", "equal_headings")),
        make_case("five_millimetres", [[0, 0, 5, 0.25], [0.003, 0.004, 5, 0.254]], DEFAULT, [0.875]),
        make_case("heading_below_quarter_pi_reduced_negative", [[0, 0, 5, 0], [0.3, 0, 5, 0.4]], DEFAULT, [0.5]),
        make_case("heading_below_quarter_pi_cruise", [[0, 0, 5, 0.1], [0.1, 0, 5, 0.7]], DEFAULT, [-0.75]),
        make_case("heading_above_quarter_pi_cruise", [[0, 0, 5, 0.2], [1, 1, 5, -1.3]], DEFAULT, [0.375]),
        make_case("heading_above_quarter_pi_reduced_negative", [[0, 0, 5, 0], [1, 0.5, 5.25, 1.2]], limits_with(w=2.0, a=2.0),
                  [-1.0]),
        make_case("seam", [[0, 0, 5, 3.1], [0.2, 0, 5, -3.1]], limits_with(w=0.3, a=0.5), [0.25], boundary=("seam",)),
        make_case("seam_the_other_way", [[0, 0, 5, -3.1], [0, 0.2, 5, 3.1]], limits_with(w=0.3, a=0.5), [0.25],
                  boundary=("seam",)),
        make_case("unwrapped_beyond_two_pi", [[0, 0, 5, 7.0], [0.5, 0.5, 5, 8.2], [1, 0, 5.5, 9.9], [1.5, 0.5, 5, 9.5]], DEFAULT,
                  [0.5, -0.25, 0.75]),
        make_case("unwrapped_below_minus_two_pi", [[0, 0, 5, -9.5], [0.5, 0.5, 5, -10.4], [0.5, 0.6, 5, -13.0]], DEFAULT,
                  [0.5, 1.0]),
        make_case("relaxed_heading", [[0, 0, 5, 0], [0.5, 0.25, 5, 2.5], [0.5, 0.25, 7, -0.5]], limits_with(w=FLT_MAX, a=FLT_MAX),
                  [0.5, -0.5]),
        make_case("equal_headings", [[0, 0, 5, 1.25], [2, 1, 5.5, 1.25], [2, 1.5, 8, 1.25]], DEFAULT, [0.25, 0.5],
                  boundary=("equal_headings",)),
        make_case("all_four_terms_one_path",
                  [[0, 0, 5, 0], [3, 0, 5.5, 0.1], [3.5, 0, 8, 0.2], [3.5, 0.004, 8, 0.2], [3.6, 0, 8, 1.6], [6, 1, 8.5, 1.7]], DEFAULT,
                  [0.5, -0.25, 1.0, 0.75, -0.5], boundary=("equal_headings",)),
    ]
    cases += [random_path(seed, 6) for seed in (1, 2, 3)]
    terms = {t for c in cases for t in c["term"]}
    assert terms == {0, 1, 2, 3}, terms
    heading = [(c["cruise"][j], c["acc"][j]) for c in cases for j, t in enumerate(c["term"]) if t == eu.HEADING]
    assert set(heading) == {(False, False), (True, False), (True, True), (False, True)}, set(heading)
    with open(OUT, "w") as f:
        json.dump(dict(generator="tests/golden/gen_estimate_cases.py", digits=mp.mp.dps, step=str(STEP), cases=cases), f,
                  separators=(",", ":"))
        f.write("\n")
    n = sum(len(c["term"]) for c in cases)
    print("%d cases, %d segments, %d bytes" % (len(cases), n, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()

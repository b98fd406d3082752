#!/usr/bin/env python3
"""Generate tests/golden/baca_cases.json: 60-digit values and gradients of the Baca segment-time estimate, for
mrs_tg_plan_estimate_times_baca and mrs_tg_plan_estimate_times_baca_vjp (csrc/mrs_tg_baca.hpp).

The ground truth is NOT the table of the header: it is central differences (step 1e-20) of L = sum_i g_i t_i over an
exact-arithmetic restatement of estimateSegmentTimesBaca AS THE REFERENCE WRITES IT -- atan2, the three limits over sin or cos
of the inclination, the normalised neighbour vectors and their clamped dot products, the two acceleration times against
sqrt(2 distance / a_max), its jerk times that enter nothing, its max_velocity_time that is overwritten, the floor, the wrapped
heading difference, 1.5 (t_vel + t_acc) -- in every waypoint coordinate and in limits 0 .. 7, with every branch decided by the
exact values.  Waypoints, limits and upstreams are taken as exact doubles; upstreams are dyadic.  The header's closed forms are
evaluated at 60 digits beside it only to (a) assert that the two agree to 1e-30 and (b) record, per output entry, the sum of
the absolute values of its addends, counted before any cancellation at the granularity at which partials() rounds: u2/|w| and
(u1.u2) u1/|w| are two addends, and c X with c = 1 - dot counts |X| + |dot X|.

The bound of the tests is K 2^-53 sum|addends| with K = 10 x the roundings on the longest chain of the header.  That chain, for
a waypoint entry: d = e - s (1), its squares (2), their sum (3, 4), the root D (5), u = d / D (6), a product of the dot (7), its
sum (8, 9), c = 1 - dot (10), c f1 (11; f1 = (v_max/a_max)(rho_a - rho_v) is ready after 9), added second of the eleven
addends of an end-part (12 .. 21), times G (22), added second of a vertex's four parts (23, 24, 25).  25 roundings, K = 250.
(A limit entry's chain is 16 roundings to the segment's part and one more per segment of the path: 23 at S = 7.)

Margins.  Every segment stays at least 1e-3 (relative) away from every branch boundary -- |inclination| against each of the
three atan2(L_v, L_h), each acceleration time against the cap, each corner's cosine against 0, the time against 0.01, the
heading term against the time, ang against 2 w^2/a, pi/4 and pi -- except where the boundary is the point of the case
("boundary" names it): a right angle (the cosine is exactly 0: not clamped, and held so while differencing) and a coincident
pair (its unit vector is the zero vector at the base point and is held so while differencing, as the header holds it).

Run from the repo root:  python3 tests/golden/gen_baca_cases.py   (a minute)
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from tests import baca_util as bu  # noqa: E402

mp.mp.dps = 60
STEP = mp.mpf("1e-20")
MARGIN = 1e-3
OUT = bu.FIXTURES
FLT_MAX = bu.FLT_MAX
DEFAULT = [2.0, 2.0, 1.0, 2.0, 2.0, 2.0, 20.0, 20.0, 20.0]
FLOOR_TIME = mp.mpf("0.01")
ZERO3 = [mp.mpf(0)] * 3
assert bu.CHAIN_ROUNDINGS == 25


class MarginError(AssertionError):
    pass


def norm3(v):
    return mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def exact_segment(w, i, lim, frozen, hold=None):
    """estimateSegmentTimesBaca's loop body for segment i, every quantity an mpf.  frozen: the segments whose length is zero at
    the base point (their unit vector is the zero vector); hold: decisions of the base point to keep (boundary cases only)"""
    S = len(w) - 1
    v_h, v_v, w_hdg, a_h, a_v, a_hdg, j_h, j_v = lim[:8]
    dec = {}

    def decide(name, value):
        dec[name] = bool(value) if hold is None else hold[name]
        return dec[name]

    def unit(seg):
        a, b = w[seg], w[seg + 1]
        v = [b[k] - a[k] for k in range(3)]
        n = norm3(v)
        if seg in frozen:
            return list(ZERO3), mp.mpf(0)
        return ([x / n for x in v] if n * n > 0 else v), n

    start, end = w[i], w[i + 1]
    d = [end[k] - start[k] for k in range(3)]
    distance = norm3(d)
    horizontal = mp.sqrt(d[0] ** 2 + d[1] ** 2)
    inclinator = mp.atan2(d[2], horizontal)

    def limit(name, lv, lh):
        thr = mp.atan2(lv, lh)
        if decide(name, inclinator > thr or inclinator < -thr):
            return abs(lv / mp.sin(inclinator)), thr
        return abs(lh / mp.cos(inclinator)), thr

    v_max, thr_v = limit("v_vertical", v_v, v_h)
    a_max, thr_a = limit("a_vertical", a_v, a_h)
    j_max, thr_j = limit("j_vertical", j_v, j_h)
    acceleration_time_1 = acceleration_time_2 = jerk_time_1 = jerk_time_2 = mp.mpf(0)
    full = (v_max / a_max) + (a_max / j_max)
    u2, _ = unit(i)
    dot1 = dot2 = None
    u1 = u3 = list(ZERO3)
    n1 = n3 = mp.mpf(0)
    if i >= 1:
        u1, n1 = unit(i - 1)
        dot1 = sum(u1[k] * u2[k] for k in range(3))
        scalar = mp.mpf(0) if decide("dot1_clamped", dot1 < 0) else dot1
        acc_1_coeff = 1 - scalar
        acceleration_time_1 = acc_1_coeff * full
        jerk_time_1 = acc_1_coeff * (2 * (a_max / j_max))
    if i == 0:
        acceleration_time_1 = full
        jerk_time_1 = 2 * (a_max / j_max)
    if i == S - 1:
        acceleration_time_2 = full
        jerk_time_2 = 2 * (a_max / j_max)
    if i < S - 1:
        u3, n3 = unit(i + 1)
        dot2 = sum(u2[k] * u3[k] for k in range(3))
        scalar = mp.mpf(0) if decide("dot2_clamped", dot2 < 0) else dot2
        acc_2_coeff = 1 - scalar
        acceleration_time_2 = acc_2_coeff * full
        jerk_time_2 = acc_2_coeff * (2 * (a_max / j_max))
    t1_raw, t2_raw = acceleration_time_1, acceleration_time_2
    cap = mp.sqrt(2 * distance / a_max)
    if decide("t1_capped", acceleration_time_1 > cap):
        acceleration_time_1 = cap
    if jerk_time_1 > mp.sqrt(2 * v_max / j_max):
        jerk_time_1 = mp.sqrt(2 * v_max / j_max)
    if decide("t2_capped", acceleration_time_2 > cap):
        acceleration_time_2 = cap
    if jerk_time_2 > mp.sqrt(2 * v_max / j_max):
        jerk_time_2 = mp.sqrt(2 * v_max / j_max)
    distance_due_acceleration = a_max * acceleration_time_1 ** 2 + a_max * acceleration_time_2 ** 2
    if distance > distance_due_acceleration:
        max_velocity_time = (distance - distance_due_acceleration) / v_max
    else:
        max_velocity_time = distance_due_acceleration / v_max
    max_velocity_time = distance / v_max
    t = max_velocity_time + acceleration_time_1 + acceleration_time_2
    t_dist = t
    if decide("floor", t < FLOOR_TIME):
        t = FLOOR_TIME
    two_pi = 2 * mp.pi
    delta = (start[3] - end[3] + mp.pi) % two_pi - mp.pi     # start minus end in [-pi, pi)
    ang = abs(delta)
    tv = ta = mp.mpf(0)
    relaxed = not (w_hdg < FLT_MAX and a_hdg < FLT_MAX)
    ang_cruise = None
    if not relaxed:
        ang_cruise = 2 * (w_hdg * w_hdg) / a_hdg
        reduced = (ang - ang_cruise) / w_hdg
        if decide("cruise", not reduced < 0):
            tv = reduced
        else:
            tv = ang / w_hdg
        if decide("acc", ang > mp.pi / 4):
            ta = 2 * (w_hdg / a_hdg)
    else:
        decide("cruise", False)
        decide("acc", False)
    hf = mp.mpf("1.5") * (tv + ta)
    if decide("heading", hf > t):
        t = hf
    for name in ("dot1_clamped", "dot2_clamped"):
        dec.setdefault(name, False)
    flags = sum(bit for name, bit in (("v_vertical", 1), ("a_vertical", 2), ("j_vertical", 4), ("t1_capped", 8), ("t2_capped", 16),
                                      ("dot1_clamped", 32), ("dot2_clamped", 64), ("floor", 128), ("heading", 256), ("cruise", 512),
                                      ("acc", 1024)) if dec[name])
    return dict(t=t, flags=flags, dec=dec, d=d, D=distance, h=horizontal, inclinator=inclinator, thr=(thr_v, thr_a, thr_j),
                t1_raw=t1_raw, t2_raw=t2_raw, cap=cap, t_dist=t_dist, hf=hf, ang=ang, delta=delta, ang_cruise=ang_cruise,
                relaxed=relaxed, u1=u1, u2=u2, u3=u3, n1=n1, n3=n3, dot1=dot1, dot2=dot2, has_pre=i >= 1, has_post=i < S - 1)


def signature(x):
    """the decisions the value depends on"""
    if x["dec"]["heading"]:
        return ("heading", x["dec"]["cruise"], x["dec"]["acc"])
    if x["dec"]["floor"]:
        return ("floor",)
    return tuple(sorted((k, v) for k, v in x["dec"].items() if k not in ("cruise", "acc")))


def closed_form(x, lim, g):
    """the header's table at 60 digits -> addends (each times g) of pre [3], start [4], end [4], post [3], lim [9], and beside
    every addend its weight in sum|addends| (c X with c = 1 - dot: |X| + |dot X|)"""
    parts = dict(pre=[[] for _ in range(3)], start=[[] for _ in range(4)], end=[[] for _ in range(4)],
                 post=[[] for _ in range(3)], lim=[[] for _ in range(9)])

    def add(where, k, value, weight=None):
        parts[where][k].append((g * value, abs(g) * (abs(value) if weight is None else weight)))

    dec = x["dec"]
    if dec["heading"]:
        w, a = lim[2], lim[5]
        sign = mp.mpf(1 if x["delta"] > 0 else -1 if x["delta"] < 0 else 0)
        add("end", 3, -mp.mpf("1.5") * sign / w)
        add("start", 3, mp.mpf("1.5") * sign / w)
        add("lim", 2, -mp.mpf("1.5") * x["ang"] / (w * w))
        if dec["cruise"]:
            add("lim", 2, -mp.mpf("1.5") * 2 / a)
            add("lim", 5, mp.mpf("1.5") * 2 * w / (a * a))
        if dec["acc"]:
            add("lim", 2, mp.mpf("1.5") * 2 / a)
            add("lim", 5, -mp.mpf("1.5") * 2 * w / (a * a))
        return parts
    if dec["floor"]:
        return parts
    d, D, h = x["d"], x["D"], x["h"]

    def regime(vertical, group):
        index = 3 * group + (1 if vertical else 0)
        c = lim[index]
        if vertical:
            q, gq = abs(d[2]), [mp.mpf(0), mp.mpf(0), mp.mpf(1 if d[2] > 0 else -1)]
        else:
            q, gq = h, [d[0] / h, d[1] / h, mp.mpf(0)]
        return dict(index=index, c=c, q=q, gq=gq, rho=[v / q for v in gq], value=c * D / q)

    V, A, J = regime(dec["v_vertical"], 0), regime(dec["a_vertical"], 1), regime(dec["j_vertical"], 2)
    r_va, r_aj = V["value"] / A["value"], A["value"] / J["value"]
    full = r_va + r_aj
    half_cap = mp.sqrt(2 * D / A["value"]) / 2
    sides = ((dec["t1_capped"], x["has_pre"] and not dec["t1_capped"] and not dec["dot1_clamped"], x["dot1"], x["u1"], x["n1"], "pre", 1),
             (dec["t2_capped"], x["has_post"] and not dec["t2_capped"] and not dec["dot2_clamped"], x["dot2"], x["u3"], x["n3"], "post", -1))
    u2 = x["u2"]
    for k in range(3):
        add("end", k, V["gq"][k] / V["c"])
        add("start", k, -V["gq"][k] / V["c"])
    add("lim", V["index"], -(V["q"] / V["c"]) / V["c"])
    for capped, smooth, dot, un, nn, far, sgn in sides:
        c = 1 - dot if smooth else mp.mpf(1)
        spread = (1 + abs(dot)) if smooth else mp.mpf(1)   # |X| + |dot X| over |X|
        if capped:
            for k in range(3):
                add("end", k, half_cap * A["rho"][k])
                add("start", k, -half_cap * A["rho"][k])
            add("lim", A["index"], -half_cap / A["c"])
            continue
        for k in range(3):
            f1 = r_va * (A["rho"][k] - V["rho"][k])
            f2 = r_aj * (J["rho"][k] - A["rho"][k])
            for f in (f1, f2):
                add("end", k, c * f, spread * abs(f))
                add("start", k, -c * f, spread * abs(f))
            if smooth and D * D > 0:       # the dot through d = e - s: dc/de = -(un - dot u2)/D, dc/ds its negative
                add("end", k, -full * un[k] / D)
                add("end", k, full * dot * u2[k] / D)
                add("start", k, full * un[k] / D)
                add("start", k, -full * dot * u2[k] / D)
            if smooth and nn * nn > 0:     # the dot through the neighbour: pre side dc/dpre = (u2 - dot u1)/n1, dc/ds its negative;
                near = "start" if far == "pre" else "end"   # post side dc/dpost = -(u2 - dot u3)/n3, dc/de its negative
                add(far, k, sgn * full * u2[k] / nn)
                add(far, k, -sgn * full * dot * un[k] / nn)
                add(near, k, -sgn * full * u2[k] / nn)
                add(near, k, sgn * full * dot * un[k] / nn)
        add("lim", V["index"], c * r_va / V["c"], spread * r_va / V["c"])
        add("lim", A["index"], -c * r_va / A["c"], spread * r_va / A["c"])
        add("lim", A["index"], c * r_aj / A["c"], spread * r_aj / A["c"])
        add("lim", J["index"], -c * r_aj / J["c"], spread * r_aj / J["c"])
    return parts


def check_margins(name, j, x, boundary):
    def away(a, b, what):
        m = max(abs(a), abs(b))
        if not (m > 0 and abs(a - b) / m >= MARGIN):
            raise MarginError((name, j, what, float(a), float(b)))
    if x["D"] == 0:
        assert "coincident" in boundary, (name, j)
        return
    for thr, what in zip(x["thr"], "vaj"):
        away(abs(x["inclinator"]), thr, "inclination against atan2 of " + what)
    away(x["t1_raw"], x["cap"], "t1 against the cap")
    away(x["t2_raw"], x["cap"], "t2 against the cap")
    for dot, what in ((x["dot1"], "dot1"), (x["dot2"], "dot2")):
        if dot is not None and not ("right_angle" in boundary or "coincident" in boundary):
            if abs(dot) < MARGIN:
                raise MarginError((name, j, what, float(dot)))
    away(x["t_dist"], FLOOR_TIME, "the time against the floor")
    if not x["relaxed"]:
        away(x["hf"], max(x["t_dist"], FLOOR_TIME), "the heading term against the time")
        away(x["ang"], x["ang_cruise"], "ang against 2 w^2 / a")
        away(x["ang"], mp.pi / 4, "ang against pi/4")
        away(x["ang"], mp.pi, "ang against the seam")


def make_case(name, waypoints, limits, upstream, boundary=()):
    w = [[mp.mpf(float(v)) for v in row] for row in waypoints]
    lim = [mp.mpf(float(v)) for v in limits]
    g = [mp.mpf(float(v)) for v in upstream]
    S = len(w) - 1
    assert len(g) == S and all(float(v) * 64 == round(float(v) * 64) for v in upstream)
    frozen = {j for j in range(S) if all(w[j][k] == w[j + 1][k] for k in range(3))}
    assert bool(frozen) == ("coincident" in boundary), name
    segs = [exact_segment(w, j, lim, frozen) for j in range(S)]
    for j, x in enumerate(segs):
        check_margins(name, j, x, boundary)
        if "right_angle" in boundary:
            assert x["dot1"] == 0 or x["dot2"] == 0, name

    def loss(wq, lq):
        total = mp.mpf(0)
        for j in range(S):
            y = exact_segment(wq, j, lq, frozen)
            if signature(y) != signature(segs[j]):
                assert boundary, (name, j, signature(y), signature(segs[j]))
                y = exact_segment(wq, j, lq, frozen, hold=segs[j]["dec"])
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
    for k in range(8):
        if lim[k] >= FLT_MAX:
            continue   # (a relaxed limit: the estimate does not depend on it)
        up, dn = list(lim), list(lim)
        up[k] += STEP
        dn[k] -= STEP
        gl[k] = (loss(w, up) - loss(w, dn)) / (2 * STEP)
    # the header's table: agreement, and the sums of |addends|
    cw = [[mp.mpf(0)] * 4 for _ in range(S + 1)]
    sw = [[mp.mpf(0)] * 4 for _ in range(S + 1)]
    cl, sl = [mp.mpf(0)] * 9, [mp.mpf(0)] * 9
    for j, x in enumerate(segs):
        parts = closed_form(x, lim, g[j])
        for where, vertex in (("pre", j - 1), ("start", j), ("end", j + 1), ("post", j + 2)):
            for k, addends in enumerate(parts[where]):
                assert 0 <= vertex <= S or not addends, (name, j, where)
                for value, weight in addends:
                    cw[vertex][k] += value
                    sw[vertex][k] += weight
        for k, addends in enumerate(parts["lim"]):
            for value, weight in addends:
                cl[k] += value
                sl[k] += weight
    for v in range(S + 1):
        for k in range(4):
            assert abs(cw[v][k] - gw[v][k]) <= mp.mpf("1e-30") * (1 + sw[v][k]), (name, v, k, cw[v][k], gw[v][k])
    for k in range(9):
        assert abs(cl[k] - gl[k]) <= mp.mpf("1e-30") * (1 + sl[k]), (name, k, cl[k], gl[k])
    assert gl[8] == 0 and sl[8] == 0
    f = lambda v: float(v)   # noqa: E731
    return dict(name=name, boundary=list(boundary), waypoints=[[float(v) for v in r] for r in waypoints],
                limits=[float(v) for v in limits], upstream=[float(v) for v in upstream], flags=[x["flags"] for x in segs],
                value=[f(x["t"]) for x in segs], grad_waypoints=[[f(v) for v in r] for r in gw], grad_limits=[f(v) for v in gl],
                scale_waypoints=[[f(v) for v in r] for r in sw], scale_limits=[f(v) for v in sl])


def limits_with(**kw):
    lim = list(DEFAULT)
    for k, v in kw.items():
        lim[dict(v_h=0, v_v=1, w=2, a_h=3, a_v=4, a=5, j_h=6, j_v=7)[k]] = v
    return lim


def random_path(name, seed, S, draw_limits):
    """box-like waypoints, limits drawn from [0.3, 4] or the default ones, re-drawn until every segment keeps the margins"""
    for attempt in range(400):
        rng = np.random.default_rng(seed * 1000 + attempt)
        w = np.column_stack([rng.uniform(-4, 4, S + 1), rng.uniform(-4, 4, S + 1), rng.uniform(1, 6, S + 1),
                             np.cumsum(rng.uniform(-1.6, 1.6, S + 1))])
        lim = rng.uniform(0.3, 4.0, 9) if draw_limits else np.array(DEFAULT)
        try:
            return make_case(name, w, lim, bu.dyadic(rng, S))
        except MarginError:
            continue
    raise RuntimeError("no draw kept the margins")


def main():
    slow_heading = dict(w=0.3, a=0.5)
    # thr_v = atan(1/2), thr_a = atan(1), thr_j = atan(2): an inclination between two of them splits the three regimes
    split = limits_with(v_h=2.0, v_v=1.0, a_h=2.0, a_v=2.0, j_h=2.0, j_v=4.0)
    cases = [
        random_path("one_segment", 11, 1, False),
        random_path("two_segments", 12, 2, False),
        random_path("three_segments", 13, 3, False),
        random_path("four_segments", 14, 4, False),
        random_path("seven_segments", 15, 7, False),
        # h = 4: dz = 2.8 is 35 degrees (v alone vertical), dz = 5.6 is 54.5 degrees (v and a), dz = 1 is 14 degrees (none)
        make_case("v_alone_vertical", [[0, 0, 1, 0], [4, 0, 3.8, 0.1], [8, 1, 4.8, 0.2]], split, [0.75, 0.5]),
        make_case("a_alone_vertical", [[0, 0, 1, 0], [4, 0, 3.8, 0.1], [8, 1, 4.8, 0.2]],
                  limits_with(v_h=2.0, v_v=2.0, a_h=2.0, a_v=1.0, j_h=2.0, j_v=4.0), [-0.5, 0.25]),
        make_case("j_alone_vertical", [[0, 0, 1, 0], [4, 0, 3.8, 0.1], [8, 1, 4.8, 0.2]],
                  limits_with(v_h=2.0, v_v=4.0, a_h=2.0, a_v=2.0, j_h=2.0, j_v=1.0), [0.625, -0.375]),
        make_case("v_and_a_vertical_descent", [[0, 0, 7, 0], [4, 0, 1.4, 0.1], [5, 3, 1.0, 0.0]], split, [0.5, 1.0]),
        make_case("right_angle", [[0, 0, 5, 0], [3, 0, 5, 0.1], [3, 4, 5, 0.2], [3, 4, 8, 0.1]], DEFAULT, [0.5, -0.75, 0.25],
                  boundary=("right_angle",)),
        make_case("reversal", [[0, 0, 5, 0], [3, 0, 5.5, 0.1], [0.5, 0.25, 5, 0.2], [4, 1, 6, 0.3]], DEFAULT, [0.5, 0.75, -0.25]),
        make_case("straight_corner", [[0, 0, 5, 0], [2, 1, 5.5, 0.1], [4, 2, 6, 0.2], [8, 4, 7, 0.1]], DEFAULT, [0.5, -0.5, 0.75]),
        make_case("both_caps", [[0, 0, 5, 0], [0.4, 0.3, 5, 0.1]], DEFAULT, [0.75]),
        make_case("one_cap_only", [[0, 0, 5, 0], [0.64, 0, 5, 0.1], [2.64, 3.5, 5, 0.2]], DEFAULT, [0.5, -0.25]),
        make_case("no_cap", [[0, 0, 5, 0], [6, 0, 5, 0.1], [12, 8, 6, 0.2]], DEFAULT, [-0.5, 0.25]),
        make_case("coincident_in_the_middle", [[0, 0, 5, 0], [3, 1, 5.5, 0.1], [3, 1, 5.5, 0.1], [5, 4, 6, 0.3], [9, 4, 6, 0.2]], DEFAULT,
                  [0.5, 0.25, -0.75, 0.5], boundary=("coincident",)),
        make_case("coincident_at_the_end", [[0, 0, 5, 0], [3, 1, 5.5, 0.1], [5, 4, 6, 0.2], [5, 4, 6, 0.2]], DEFAULT,
                  [0.5, -0.25, 0.75], boundary=("coincident",)),
        make_case("five_millimetres", [[0, 0, 5, 0], [3, 4, 5, 0.01], [3.003, 4.004, 5, 0.012], [6.003, 8.004, 5, 0.02]], DEFAULT,
                  [0.875, 0.5, -0.25]),
        make_case("five_millimetres_alone", [[0, 0, 5, 0.25], [0.003, 0.004, 5, 0.254]], DEFAULT, [0.875]),
        make_case("heading_below_quarter_pi_reduced_negative", [[0, 0, 5, 0], [0.3, 0, 5, 0.3]], limits_with(**slow_heading), [0.5]),
        make_case("heading_below_quarter_pi_cruise", [[0, 0, 5, 0.1], [0.3, 0, 5, 0.8]], limits_with(**slow_heading), [-0.75]),
        make_case("heading_above_quarter_pi_cruise", [[0, 0, 5, 0.2], [0.2, 0.2, 5, -1.3]], limits_with(**slow_heading), [0.375]),
        make_case("heading_above_quarter_pi_reduced_negative", [[0, 0, 5, 0], [0.25, 0.125, 5.0625, 1.2]], limits_with(w=2.0, a=2.0),
                  [-1.0]),
        make_case("seam", [[0, 0, 5, 3.1], [0.02, 0, 5, -3.1]], limits_with(**slow_heading), [0.25]),
        make_case("seam_the_other_way", [[0, 0, 5, -3.1], [0, 0.02, 5, 3.1]], limits_with(**slow_heading), [0.25]),
        make_case("heading_in_the_middle", [[0, 0, 5, 0], [3, 0, 5.5, 0.1], [3.2, 0.1, 5.5, 1.7], [6, 1, 6, 1.8]],
                  limits_with(**slow_heading), [0.5, 0.75, -0.5]),
        make_case("relaxed_heading", [[0, 0, 5, 0], [0.5, 0.25, 5, 2.5], [0.5, 1.25, 7, -0.5]], limits_with(w=FLT_MAX, a=FLT_MAX),
                  [0.5, -0.5]),
    ]
    cases += [random_path("limits_drawn_%d" % seed, seed, 6, True) for seed in (1, 2, 3)]
    by_name = {c["name"]: c for c in cases}
    seen = 0
    for c in cases:
        for fl in c["flags"]:
            seen |= fl
    assert seen == 2047, seen
    assert [fl & 7 for fl in by_name["v_alone_vertical"]["flags"]] == [1, 0]
    assert [fl & 7 for fl in by_name["a_alone_vertical"]["flags"]] == [2, 0]
    assert [fl & 7 for fl in by_name["j_alone_vertical"]["flags"]] == [4, 0]
    assert by_name["v_and_a_vertical_descent"]["flags"][0] & 7 == 3
    assert by_name["reversal"]["flags"][0] & 64 and by_name["reversal"]["flags"][1] & 32
    assert not any(fl & (32 | 64) for fl in by_name["right_angle"]["flags"])
    assert by_name["both_caps"]["flags"][0] & 24 == 24 and by_name["one_cap_only"]["flags"][0] & 24 == 8
    assert not any(fl & 24 for fl in by_name["no_cap"]["flags"])
    assert by_name["five_millimetres"]["flags"][1] & 384 == 128 and by_name["five_millimetres_alone"]["flags"][0] & 384 == 0
    assert by_name["coincident_in_the_middle"]["flags"][1] & 128 and by_name["coincident_at_the_end"]["flags"][2] & 128
    heading = {(fl >> 9) & 3 for c in cases for fl in c["flags"] if fl & 256}
    assert heading == {0, 1, 2, 3}, heading
    assert by_name["seam"]["flags"][0] & 256 and by_name["seam_the_other_way"]["flags"][0] & 256
    assert by_name["heading_in_the_middle"]["flags"][1] & 256 and not by_name["heading_in_the_middle"]["flags"][0] & 256
    assert not any(fl & (256 | 512 | 1024) for fl in by_name["relaxed_heading"]["flags"])
    with open(OUT, "w") as f:
        json.dump(dict(generator="tests/golden/gen_baca_cases.py", digits=mp.mp.dps, step=str(STEP), cases=cases), f,
                  separators=(",", ":"))
        f.write("\n")
    n = sum(len(c["flags"]) for c in cases)
    print("%d cases, %d segments, %d bytes" % (len(cases), n, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()

"""What the tests of the request's vertices and limits as plan steps share (mrs_tg_plan_request_vertices,
mrs_tg_plan_request_limits, csrc/mrs_tg_request.hpp): the vertex problems at the chunk edges, the branch
table of the limits, the Pythagorean edge of can_change, and the CPU harness tests/host/request_harness.cpp."""
import itertools

import numpy as np

from tests import host_harness as hh

# MRS_TG_REQ_* and MRS_TG_LIM_* (include/mrs_tg.h)
REQ_OVERRIDE, REQ_RELAX_HEADING = 1, 2
OVERRIDDEN, OVERRIDE_REFUSED, RELAXED, V_DESCENDING, A_DESCENDING, J_DESCENDING, FALLBACK = 1, 2, 4, 8, 16, 32, 64
FLT_MAX = 3.4028234663852886e+38
HOST_V = (2, 3, 4, 11, 64, 65, 129, 257)             # vertices of a path on the CPU: the chunk of 64 and two of them
SPEED_FACTOR, ACCEL_FACTOR = 0.75, 0.5               # the fallback's factors in the tests: products with them are exact


def vertex_problem(rng, V, d, has_state, pi_steps=False):
    """one path: raw headings and the state's heading in +-3 pi, stop flags at random, the ends included; pi_steps: every heading
    exactly pi from the one before it, the sign at random (the step at which the unwrap chooses a direction)"""
    raw = rng.uniform(-5.0, 5.0, size=(V, 4))
    raw[:, 3] = rng.uniform(-3.0 * np.pi, 3.0 * np.pi, size=V)
    state = rng.uniform(-2.0, 2.0, size=(4, 4))
    state[0, 3] = rng.uniform(-3.0 * np.pi, 3.0 * np.pi)
    if pi_steps:
        raw[0, 3] = state[0, 3] + np.pi if has_state else raw[0, 3]
        for i in range(1, V):
            raw[i, 3] = raw[i - 1, 3] + (np.pi if rng.random() < 0.5 else -np.pi)
    stop = (rng.random(V) < 0.4).astype(np.uint8)
    return dict(V=V, d=d, has=int(has_state), state=state, raw=raw, stop=stop)


def vertex_problems(seed=20):
    rng = np.random.default_rng(seed)
    out = []
    for V, d, has in itertools.product(HOST_V, (2, 3, 4), (0, 1)):
        out.append(vertex_problem(rng, V, d, has))
        out.append(vertex_problem(rng, V, d, has, pi_steps=True))
    return out


def state_block(velocity=(0, 0, 0), acceleration=(0, 0, 0), jerk=(0, 0, 0), heading=0.25):
    s = np.zeros((4, 4))
    s[0, 3] = heading
    s[1, :3], s[2, :3], s[3, :3] = velocity, acceleration, jerk
    s[1:, 3] = (0.125, -0.25, 0.5)
    return s


# override: velocity h, v; acceleration h, v; jerk h, v.  The state `below` is strictly inside all six; ABOVE[k] leaves the k-th
# comparison of can_change (in the reference's order) and only that one
OVERRIDE = np.array([6.0, 3.0, 5.0, 2.5, 40.0, 30.0])
BELOW = dict(velocity=(3.0, 4.0, 2.0), acceleration=(1.5, 2.0, -2.0), jerk=(12.0, 16.0, 25.0))      # hypot 5, 2.5, 20
ABOVE = [dict(BELOW, velocity=(6.0, 8.0, 2.0)), dict(BELOW, acceleration=(6.0, 8.0, -2.0)), dict(BELOW, jerk=(48.0, 64.0, 25.0)),
         dict(BELOW, velocity=(3.0, 4.0, -3.5)), dict(BELOW, acceleration=(1.5, 2.0, 2.75)), dict(BELOW, jerk=(12.0, 16.0, -31.0))]


def constraints(pairs):
    """c[12] with the three vertical pairs (speed, acceleration, jerk) ordered as pairs says: '<' ascending below descending,
    '=' equal, '>' ascending above descending"""
    c = np.array([8.0, 4.0, 60.0, 0, 0, 0, 0, 0, 0, 1.0, 2.0, 20.0])
    for k, (rel, base) in enumerate(zip(pairs, (4.0, 2.0, 48.0))):
        c[3 + 2 * k], c[4 + 2 * k] = {"<": (base, base + 1.0), "=": (base, base), ">": (base + 1.0, base)}[rel]
    return c


def limits_table():
    """the branch table as rows dict(flags, has, fallback, c, o, state, expect): override off / on x state none / below / above
    each of the six thresholds in turn x relax x fallback x each vertical pair asc <, =, > desc.  expect: the branch word."""
    rows = []
    states = [("none", None), ("below", BELOW)] + [("above%d" % k, a) for k, a in enumerate(ABOVE)]
    for over, (name, st), relax, fallback, rel in itertools.product((0, 1), states, (0, 1), (0, 1), "<=>"):
        pairs = {"<": "<=>", "=": "=><", ">": "><="}[rel]       # every pair meets every relation over the three values of rel
        expect = (FALLBACK if fallback else 0) | (RELAXED if relax else 0)
        for bit, r in zip((V_DESCENDING, A_DESCENDING, J_DESCENDING), pairs):
            expect |= bit if r == ">" else 0
        if over:
            refused = not fallback and name.startswith("above")
            expect |= OVERRIDE_REFUSED if refused else OVERRIDDEN
        rows.append(dict(flags=(REQ_OVERRIDE if over else 0) | (REQ_RELAX_HEADING if relax else 0), has=int(st is not None),
                         fallback=fallback, c=constraints(pairs), o=OVERRIDE.copy(),
                         state=state_block(**st) if st is not None else state_block(), expect=expect, name=name))
    return rows


def edge_rows():
    """the strict < at the edge, where hypot is exact on every side: velocity (3, 4) against an override of 5.0 is refused,
    against the next double above 5.0 accepted; the same for |z| against the vertical override"""
    up = float(np.nextafter(5.0, np.inf))
    rows = []
    for slot, kind in ((0, "velocity"), (2, "acceleration"), (4, "jerk")):
        for value, expect in ((5.0, OVERRIDE_REFUSED), (up, OVERRIDDEN)):
            o = np.array([100.0] * 6)
            o[slot] = value
            st = state_block(**{kind: (3.0, 4.0, 1.0)})
            rows.append(dict(flags=REQ_OVERRIDE, has=1, fallback=0, c=constraints("<<<"), o=o, state=st, expect=expect, name="edge"))
    for slot, kind in ((1, "velocity"), (3, "acceleration"), (5, "jerk")):
        for value, expect in ((5.0, OVERRIDE_REFUSED), (up, OVERRIDDEN)):
            o = np.array([100.0] * 6)
            o[slot] = value
            st = state_block(**{kind: (1.0, 1.0, -5.0)})
            rows.append(dict(flags=REQ_OVERRIDE, has=1, fallback=0, c=constraints("<<<"), o=o, state=st, expect=expect, name="edge"))
    return rows


def expected_limits(row):
    """lim[9] of a table row, from its expected branch word (numpy)"""
    c, o, w = row["c"], row["o"], row["expect"]
    lim = np.array([c[0], c[4] if w & V_DESCENDING else c[3], c[9], c[1], c[6] if w & A_DESCENDING else c[5], c[10],
                    c[2], c[8] if w & J_DESCENDING else c[7], c[11]])
    if w & OVERRIDDEN:
        lim[[0, 1, 3, 4, 6, 7]] = o
    if w & RELAXED:
        lim[[2, 5, 8]] = FLT_MAX
    if w & FALLBACK:
        lim[[0, 1]] *= SPEED_FACTOR
        lim[[3, 4]] *= ACCEL_FACTOR
    return lim


# ---- the CPU harness -----------------------------------------------------------------------------------------------------------

def build_harness(tmp_path, sanitize=False):
    return hh.build("request_harness.cpp", tmp_path, sanitize=sanitize)


def _vertex_line(letter, q):
    return "%s %d %d %d %s %s %s\n" % (letter, q["V"], q["d"], q["has"], hh.fmt(q["state"]), hh.fmt(q["raw"]),
                                       " ".join(str(int(s)) for s in q["stop"]))


def _limit_line(letter, r):
    return "%s %d %d %d %r %r %s %s %s\n" % (letter, r["flags"], r["has"], r["fallback"], SPEED_FACTOR, ACCEL_FACTOR, hh.fmt(r["c"]),
                                             hh.fmt(r["o"]), hh.fmt(r["state"]))


def _hex(tokens):
    return np.array([float.fromhex(t) for t in tokens], dtype=np.float64)


def run_vertices(exe, problems):
    """-> [len(problems)][4]: 1 where waypoints, mask, values and the in-place waypoints have the bytes of the harness's restatement"""
    out = hh.run(exe, [_vertex_line("V", q) for q in problems], len(problems))
    return np.array([[int(t) for t in line.split()] for line in out], dtype=np.int64)


def run_limits(exe, rows):
    """-> (branch [n], lim [n][9] of the header, lim [n][9] of the restatement of the reference's lines)"""
    out = hh.run(exe, [_limit_line("L", r) for r in rows], len(rows))
    branch, new, ref = [], [], []
    for line in out:
        a, b = line.split("|")
        a = a.split()
        branch.append(int(a[0]))
        new.append(_hex(a[1:]))
        ref.append(_hex(b.split()))
    return np.array(branch, dtype=np.int32), np.array(new).reshape(-1, 9), np.array(ref).reshape(-1, 9)


def run_backward(exe, letter, items):
    """-> per item (the backward pass's gradient, the central differences' gradient)"""
    line_of = _vertex_line if letter == "G" else _limit_line
    res = []
    for line in hh.run(exe, [line_of(letter, q) for q in items], len(items)):
        a, b = line.split("|")
        res.append((_hex(a.split()), _hex(b.split())))
    return res


def dyadic_vertex_problem(rng, V, d, has_state):
    """a vertex problem for central differences with a step of 0.25: x, y, z and the state's rows are multiples of 1/8, so the
    differences of the copies are exact; every heading is within 2 rad of the one before it modulo 2 pi (the first of the state's
    where there is one), so no perturbed heading changes the multiple of 2 pi its unwrap adds"""
    q = vertex_problem(rng, V, d, has_state)
    q["raw"][:, :3] = np.round(q["raw"][:, :3] * 8.0) / 8.0
    q["state"][1:] = np.round(q["state"][1:] * 8.0) / 8.0
    steps = rng.uniform(-2.0, 2.0, size=V)
    if not has_state:
        steps[0] = 0.0
    q["raw"][:, 3] = q["state"][0, 3] + np.cumsum(steps) + 2.0 * np.pi * rng.integers(-1, 2, size=V)
    return q


def backward_limit_rows():
    """the rows of the branch table the limits are differentiable at: no vertical pair is a tie, every comparison of can_change
    has a margin above the differences' step"""
    rows = []
    for r, pairs in zip(limits_table(), itertools.cycle(("<<>", "><<", "<><", ">><"))):
        expect = r["expect"] & ~(V_DESCENDING | A_DESCENDING | J_DESCENDING)
        for bit, rel in zip((V_DESCENDING, A_DESCENDING, J_DESCENDING), pairs):
            expect |= bit if rel == ">" else 0
        rows.append(dict(r, c=constraints(pairs), expect=expect))
    return rows

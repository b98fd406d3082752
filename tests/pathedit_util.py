"""What the tests of path thinning and mid-point subdivision as plan steps share (tests/test_pathedit_host.py,
tests/test_gpu_pathedit.py): the line grammar of tests/host/pathedit_harness.cpp, the oracle's mto_preprocess_path, a
restatement of the reference's insertion loop AS WRITTEN (optimize(), src/mrs_trajectory_generation.cpp:739-753: an index into a
growing list, the size tested where the loop stands) on the oracle's mto_interpolate_point, a restatement of the backward sums in
Python floats in the stated order, the fixed cases and the generators.  Nothing here needs a tolerance: thinning copies rows,
the mid-point is two roundings a coordinate and an fmod chain for the heading, the same operations on both sides."""
import math

import numpy as np

from oracle import pyoracle as po
from tests import deviation_util as du
from tests import host_harness as hh

HARNESS = "pathedit_harness.cpp"
WINDOW = 64            # pathq::kWindow: the candidates a wavefront judges at once
SCAN_CHUNK = 1024      # kPathEditScanChunk: the paths the offsets' one workgroup takes at a time
bits, same_bits, dyadic = du.bits, du.same_bits, du.dyadic


def build_harness(tmp_path, sanitize=False):
    return hh.build(HARNESS, tmp_path, sanitize=sanitize)


# ---- thinning ----------------------------------------------------------------------------------------------------------

def thin_problem(waypoints, min_distance, stop_at=None, straightener=None, name=""):
    """straightener: None (off) or (max_deviation, max_hdg_deviation)"""
    w = np.array(waypoints, dtype=np.float64).reshape(-1, 4)
    stop = np.zeros(w.shape[0], dtype=np.uint8) if stop_at is None else np.array(stop_at, dtype=np.uint8).reshape(w.shape[0])
    return dict(waypoints=w, stop_at=stop, min_distance=float(min_distance), straightener=straightener, name=name)


def _thin_line(p):
    on = p["straightener"] is not None
    dev, hdg = p["straightener"] if on else (0.0, 0.0)
    return "1 %d %r %d %r %r %s %s\n" % (p["waypoints"].shape[0], p["min_distance"], int(on), float(dev), float(hdg),
                                        hh.fmt(p["waypoints"]), hh.fmt(p["stop_at"]))


def run_thin(exe, problems, env=None):
    """per problem dict(serial, window: kept input indices; rows [n][4], stop_at [n]: policy::preprocess's result)"""
    out = hh.run(exe, [_thin_line(p) for p in problems], len(problems), env=env)
    res = []
    for line in out:
        x = line.split()
        n = int(x[0])
        serial = np.array([int(v) for v in x[1:1 + n]], dtype=np.int64)
        x = x[1 + n:]
        m = int(x[0])
        window = np.array([int(v) for v in x[1:1 + m]], dtype=np.int64)
        x = x[1 + m:]
        k = int(x[0])
        stop = np.array([int(v) for v in x[1:1 + k]], dtype=np.uint8)
        rows = np.array([float(v) for v in x[1 + k:]]).reshape(k, 4)
        res.append(dict(serial=serial, window=window, rows=rows, stop_at=stop))
    return res


def oracle_thin(p):
    """mto_preprocess_path -> (rows [n][4], stop_at [n])"""
    w = po._f64(p["waypoints"])
    stop = np.ascontiguousarray(p["stop_at"], dtype=np.uint8)
    on = p["straightener"] is not None
    dev, hdg = p["straightener"] if on else (0.0, 0.0)
    prm = po.default_policy(min_waypoint_distance=p["min_distance"], path_straightener_enabled=int(on),
                            path_straightener_max_deviation=float(dev), path_straightener_max_hdg_deviation=float(hdg))
    out = np.zeros_like(w)
    stop_out = np.zeros(w.shape[0], dtype=np.uint8)
    u8 = po.C.POINTER(po.C.c_uint8)
    n = po.lib().mto_preprocess_path(po._dp(w), stop.ctypes.data_as(u8), w.shape[0], po.C.byref(prm), po._dp(out),
                                     stop_out.ctypes.data_as(u8))
    return out[:n].copy(), stop_out[:n].copy()


def path_from_kept(V, kept, rng, spacing=10.0, heading=True):
    """a path of V vertices of which a thinning at min_waypoint_distance = spacing / 2 keeps exactly the input indices `kept`
    (0 and V - 1 among them): a kept vertex stands `spacing` further along x than the one before, the others within 0.02 of the
    kept vertex in front of them"""
    kept = sorted(set(int(k) for k in kept) | {0, V - 1})
    w = np.zeros((V, 4))
    rank = np.searchsorted(np.array(kept), np.arange(V), side="right") - 1
    w[:, 0] = spacing * rank
    is_kept = np.zeros(V, dtype=bool)
    is_kept[kept] = True
    w[~is_kept, :3] += rng.uniform(-0.01, 0.01, size=(int((~is_kept).sum()), 3))
    if heading:
        w[:, 3] = rng.uniform(-7.0, 7.0, size=V)
    return w, np.array(kept)


def fixed_thin_cases():
    """the issue's fixed cases -> list of (problem, number kept or None)"""
    rng = np.random.default_rng(11)
    cases = []
    cases.append((thin_problem([[0, 0, 1, 0.3], [0.001, 0, 1, -0.2]], 5.0, name="V2"), 2))
    cases.append((thin_problem([[0, 0, 0, 0], [3, 4, 0, 1], [30, 0, 0, 2]], 5.0, name="V3_at_threshold_kept"), 3))
    cases.append((thin_problem([[0, 0, 0, 0], [3, 4 - 1e-15, 0, 1], [30, 0, 0, 2]], 5.0, name="V3_below_threshold_dropped"), 2))
    cases.append((thin_problem([[0, 0, 0, 0], [math.nan, 0.1, 0, 1], [0.2, 0.1, 0, 2]], 5.0, name="nan_kept"), 3))
    w, kept = path_from_kept(130, [0] + list(range(101, 130)), rng)
    cases.append((thin_problem(w, 5.0, stop_at=rng.integers(0, 2, 130), name="run_of_100_in_130"), 30))
    w, kept = path_from_kept(257, [0, 256], rng)
    cases.append((thin_problem(w, 5.0, name="all_interior_dropped_257"), 2))
    # the straightener's three tests; min_waypoint_distance 0.1 never drops these vertices itself
    st = (0.2, 0.3)
    cases.append((thin_problem([[0, 0, 0, 0.1], [5, 0.1, 0, 0.1], [10, 0, 0, 0.1]], 0.1, straightener=st, name="straight_dropped"), 2))
    cases.append((thin_problem([[0, 0, 0, 0.1], [5, 0.5, 0, 0.1], [10, 0, 0, 0.1]], 0.1, straightener=st, name="off_the_line_kept"), 3))
    cases.append((thin_problem([[0, 0, 0, 1.0], [5, 0.1, 0, 0.5], [10, 0, 0, 0.5]], 0.1, straightener=st, name="first_heading_kept"), 3))
    cases.append((thin_problem([[0, 0, 0, 0.5], [5, 0.1, 0, 0.5], [10, 0, 0, 1.0]], 0.1, straightener=st, name="last_heading_kept"), 3))
    # quirk B3: the middle heading is 1.0 ABOVE both ends' -- the signed differences are -1.0 and -0.5, not above 0.3, so the
    # vertex goes; an absolute comparison would keep it
    cases.append((thin_problem([[0, 0, 0, 0.0], [5, 0.1, 0, 1.0], [10, 0, 0, 0.5]], 0.1, straightener=st, name="b3_signed_dropped"), 2))
    # ... and across the seam: 6.2 is 0.083 BELOW 0 on the circle, so diff(first, mid) = +0.083 passes as well
    cases.append((thin_problem([[0, 0, 0, 0.0], [5, 0.1, 0, 6.2], [10, 0, 0, 6.2]], 0.1, straightener=st, name="seam_dropped"), 2))
    return cases


def window_cases(rng):
    """paths whose kept vertices sit where the 64-candidate window's paths differ -> list of (V, kept): a jump from `last` ends on
    candidate lane (next - last - 1) % 64 after (next - last - 1) // 64 empty windows"""
    return [(64, [0, 63]),                          # lane 62
            (65, [0, 64]),                          # lane 63
            (66, [0, 65]),                          # the next window, lane 0
            (129, [0, 1, 64, 128]),                 # lanes 0, 62, 63
            (130, [0, 129]),                        # two empty windows, then lane 0
            (257, [0, 1, 64, 128, 199, 256]),       # lanes 0, 62, 63, the next window (lane 6), lane 56
            (257, [0, 134, 256]),                   # one `last` survives two empty windows (lane 5), then one more
            (257, [0, 256])]                        # three empty windows, lane 63


def random_clustered_path(rng, V, straight=False):
    """clusters of close vertices between long steps; with `straight` mostly along a line with headings close together, so that
    the straightener's three tests all decide"""
    w = np.zeros((V, 4))
    pos = rng.uniform(-5, 5, size=3)
    direction = rng.normal(size=3)
    direction /= np.linalg.norm(direction)
    h = rng.uniform(-math.pi, math.pi)
    for v in range(V):
        if v and rng.random() < 0.6:
            pos = pos + rng.uniform(-0.03, 0.03, size=3)          # stays in the cluster
        elif v:
            if not straight or rng.random() < 0.2:
                direction = rng.normal(size=3)
                direction /= np.linalg.norm(direction)
            pos = pos + direction * rng.uniform(0.2, 3.0) + (rng.normal(size=3) * 0.03 if straight else 0.0)
        h = h + (rng.normal() * 0.15 if straight else rng.uniform(-3, 3))
        w[v, :3], w[v, 3] = pos, h
    return w


# ---- subdivision --------------------------------------------------------------------------------------------------------

def subdivide_problem(waypoints, unsafe, first_segment, stop_at=None, name=""):
    w = np.array(waypoints, dtype=np.float64).reshape(-1, 4)
    stop = np.zeros(w.shape[0], dtype=np.uint8) if stop_at is None else np.array(stop_at, dtype=np.uint8).reshape(w.shape[0])
    return dict(waypoints=w, stop_at=stop, unsafe=np.array(unsafe, dtype=np.uint8).reshape(w.shape[0] - 1),
                first_segment=int(bool(first_segment)), name=name)


def run_subdivide(exe, problems, env=None):
    """per problem dict(rows [n][4], stop_at [n], source [n] (the path's own numbering), inserted [n])"""
    lines = ["2 %d %d %s %s %s\n" % (p["waypoints"].shape[0], p["first_segment"], hh.fmt(p["waypoints"]), hh.fmt(p["stop_at"]),
                                     hh.fmt(p["unsafe"])) for p in problems]
    out = hh.run(exe, lines, len(problems), env=env)
    res = []
    for line in out:
        x = line.split()
        n = int(x[0])
        rows = np.array([float(v) for v in x[1:1 + 4 * n]]).reshape(n, 4)
        ints = np.array([int(v) for v in x[1 + 4 * n:]], dtype=np.int64)
        assert ints.size == 3 * n
        res.append(dict(rows=rows, stop_at=ints[:n].astype(np.uint8), source=ints[n:2 * n], inserted=ints[2 * n:].astype(np.uint8)))
    return res


def oracle_midpoint(a, b, coeff=0.5):
    a, b, out = po._f64(a), po._f64(b), np.zeros(4)
    po.lib().mto_interpolate_point(po._dp(a), po._dp(b), po.C.c_double(float(coeff)), po._dp(out))   # (no argtypes declared)
    return out


def reference_subdivide(p):
    """:739-753 as written: the iterator is an index into the growing list, waypoints.size() is whatever the list holds then"""
    wps = [r.copy() for r in p["waypoints"]]
    stop = [int(s) for s in p["stop_at"]]
    safeness = [not u for u in p["unsafe"]]
    w = s = 0
    while w < len(wps) - 1:
        if not safeness[s]:
            if w > 0 or p["first_segment"] or len(wps) <= 2:
                wps.insert(w + 1, oracle_midpoint(wps[w], wps[w + 1]))
                stop.insert(w + 1, 0)
                w += 1
        s += 1
        w += 1
    return np.array(wps).reshape(-1, 4), np.array(stop, dtype=np.uint8)


def flag_patterns(S, rng):
    return dict(none=np.zeros(S, dtype=np.uint8), all=np.ones(S, dtype=np.uint8),
                alternating=(np.arange(S) % 2 == 0).astype(np.uint8), odd=(np.arange(S) % 2 == 1).astype(np.uint8),
                random=rng.integers(0, 2, S).astype(np.uint8))


def random_path(rng, V):
    w = rng.uniform(-20, 20, size=(V, 4))
    w[:, 3] = rng.uniform(-7.0, 7.0, size=V)
    return w


def seam_path():
    """heading pairs across the 0 / 2 pi seam, both ways, and a difference of exactly pi"""
    h = [0.1, 6.2, 0.05, -0.1, 3.0, 3.0 + math.pi, 2 * math.pi, 0.0]
    w = np.zeros((len(h), 4))
    w[:, 0] = np.arange(len(h))
    w[:, 3] = h
    return w


# ---- backward pass ------------------------------------------------------------------------------------------------------

def run_vjp(exe, problems, env=None):
    """problems: dicts(n_in, source [n_run] in the path's own numbering, inserted [n_run] or None, upstream [n_run][4]) ->
    dL/dwaypoints [n_in][4] each"""
    lines = []
    for p in problems:
        n_run = len(p["source"])
        ins = p["inserted"] if p["inserted"] is not None else np.zeros(n_run)
        lines.append("3 %d %d %d %s %s %s\n" % (p["n_in"], n_run, int(p["inserted"] is not None), hh.fmt(p["source"]), hh.fmt(ins),
                                                hh.fmt(p["upstream"])))
    out = hh.run(exe, lines, len(problems), env=env)
    return [np.array([float(v) for v in line.split()]).reshape(p["n_in"], 4) for p, line in zip(problems, out)]


def reference_vjp(n_in, source, inserted, upstream):
    """the stated order in Python floats: from 0.0, half the mid-point in front, the own copy, half the own mid-point"""
    g = np.zeros((n_in, 4))
    up = np.asarray(upstream, dtype=np.float64)
    ins = np.zeros(len(source), dtype=np.uint8) if inserted is None else np.asarray(inserted)
    copy_at = {int(s): r for r, s in enumerate(source) if not ins[r]}
    for v in range(n_in):
        if v not in copy_at:
            continue
        r = copy_at[v]
        for k in range(4):
            acc = 0.0
            if r > 0 and ins[r - 1]:
                acc = acc + 0.5 * float(up[r - 1, k])
            acc = acc + float(up[r, k])
            if r + 1 < len(source) and ins[r + 1]:
                acc = acc + 0.5 * float(up[r + 1, k])
            g[v, k] = acc
    return g


# ---- the chain deviation -> subdivision ---------------------------------------------------------------------------------

def run_chain(exe, problems, env=None):
    """problems: dicts(waypoints [V][4], stop_at [V], samples [n][4], first_segment, max_deviation) -> dict(is_safe, rows,
    stop_at) of devq::validate + policy::insert_midpoints"""
    lines = ["4 %d %d %d %r %s %s %s\n" % (p["waypoints"].shape[0], p["samples"].shape[0], int(p["first_segment"]),
                                          float(p["max_deviation"]), hh.fmt(p["waypoints"]), hh.fmt(p["stop_at"]),
                                          hh.fmt(p["samples"])) for p in problems]
    out = hh.run(exe, lines, len(problems), env=env)
    res = []
    for line in out:
        x = line.split()
        safe, n = int(x[0]), int(x[1])
        rows = np.array([float(v) for v in x[2:2 + 4 * n]]).reshape(n, 4)
        res.append(dict(is_safe=bool(safe), rows=rows, stop_at=np.array([int(v) for v in x[2 + 4 * n:]], dtype=np.uint8)))
    return res

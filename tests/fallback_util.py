"""What the tests of the fallback sampler as a plan step share (tests/test_fallback_host.py, tests/test_gpu_fallback.py): the
harness's line grammar, a restatement of the reference's loop AS WRITTEN (findTrajectoryFallback,
src/mrs_trajectory_generation.cpp:1327-1381: push_back by push_back, math.ceil, round; the heading through the oracle's
wrap_yaw) -- not the closed-form row index of csrc/mrs_tg_fallback.hpp, so an independent check of the row -> (segment, j) map
-- a restatement of the backward sums in Python floats in the pinned order, the explicit-time edge cases and the batches.

THE HEADING BOUND of the GPU tier, counted, not measured.  The kernel's heading is wrap_yaw(y) = atan2(2 (w z), 1 - 2 (z z)),
w = cos(y / 2), z = sin(y / 2), on a y that has the host's bits; only sin, cos and atan2 differ between the device and the host.
With u = 2^-53 (one rounding; 1 ulp <= 2 u relative), device functions of 2 ulp and host functions of 1 ulp.  These two
figures for the ROCm device library's and glibc's double sin, cos and atan2 are ASSUMED, NOT CONFIRMED: no accuracy table of
either library was checked when the count was made, and the bound stands or falls with them (the worst difference seen on an
MI355X is 0.125 of the bound).
  w, z            differ by 3 ulp = 6 u relative each
  A = 2 (w z)     6 u + 6 u + one rounding a side = 14 u relative, |A| <= 1:                            14 u
  B = 1 - 2 z z   2 z z <= 2 differs by (12 u + 2 u) * 2 = 28 u, the subtraction one rounding a side:   28 u + 2 u
  theta = atan2(A, B), A^2 + B^2 = 1 up to roundings: |d theta| <= |dA| + |dB|                         44 u
  atan2 itself    3 ulp of a value of at most pi: 6 u * pi                                              19 u
in all 63 u: HEADING_K = 64.  Headings are compared as the wrapped difference, so a flip between -pi and pi is no error."""
import math

import numpy as np

from oracle import pyoracle as po
from tests import baca_util as bu
from tests import host_harness as hh

HARNESS = "fallback_harness.cpp"
HEADING_K = 64
HEADING_BOUND = HEADING_K * 2.0 ** -53
COUNT_CLAMP = 2 ** 31
TWO_PI = 2.0 * math.pi
bits, same_bits, shapes = bu.bits, bu.same_bits, bu.shapes


def build_harness(tmp_path, sanitize=False):
    return hh.build(HARNESS, tmp_path, sanitize=sanitize)


def problem(waypoints, seg_times, dt, capacity, stop_at=None, stopping_time=2.0, upstream=None, name=""):
    w = np.array(waypoints, dtype=np.float64).reshape(-1, 4)
    S = w.shape[0] - 1
    stop = np.zeros(S + 1, dtype=np.uint8) if stop_at is None else np.array(stop_at, dtype=np.uint8).reshape(S + 1)
    up = None if upstream is None else np.array(upstream, dtype=np.float64).reshape(int(capacity), 4)
    return dict(waypoints=w, stop_at=stop, seg_times=np.array(seg_times, dtype=np.float64).reshape(S), dt=float(dt),
                capacity=int(capacity), stopping_time=float(stopping_time), upstream=up, name=name)


def run_harness(exe, problems, env=None):
    """explicit times -> per problem dict(count, n_samples, seg_first_row [S], rows [n][4], grad_waypoints [S + 1][4] or None),
    or None for a problem whose arguments the harness refuses"""
    lines = []
    for p in problems:
        S = p["waypoints"].shape[0] - 1
        lines.append("1 %d %d %r %r %d %s %s %s %s\n" % (S, p["capacity"], p["dt"], p["stopping_time"],
                                                        int(p["upstream"] is not None), hh.fmt(p["waypoints"]),
                                                        hh.fmt(p["stop_at"]), hh.fmt(p["seg_times"]),
                                                        "" if p["upstream"] is None else hh.fmt(p["upstream"])))
    out = hh.run(exe, lines, len(problems), env=env)
    res = []
    for p, line in zip(problems, out):
        if line.strip() == "invalid":
            res.append(None)
            continue
        S = p["waypoints"].shape[0] - 1
        x = line.split()
        count, n_sat = int(x[0]), int(x[1])
        first = np.array([int(v) for v in x[2:2 + S]], dtype=np.int64)
        n = min(count, p["capacity"])
        rest = np.array([float(v) for v in x[2 + S:]])
        assert rest.size == 4 * n + (4 * (S + 1) if p["upstream"] is not None else 0), (p["name"], rest.size, n, S)
        res.append(dict(count=count, n_samples=n_sat, seg_first_row=first, rows=rest[:4 * n].reshape(n, 4),
                        grad_waypoints=rest[4 * n:].reshape(S + 1, 4) if p["upstream"] is not None else None))
    return res


def run_chain_harness(exe, chains, env=None):
    """the whole findTrajectoryFallback -> per chain dict(unwrapped [S + 1], seg_times [S], count, rows [n][4]); chains:
    dicts(waypoints, stop_at, limits, relax, speed_factor, accel_factor, dt, stopping_time, capacity)"""
    lines = []
    for c in chains:
        S = c["waypoints"].shape[0] - 1
        lines.append("2 %d %d %r %r %d %r %r %s %s %s\n" % (S, c["capacity"], float(c["dt"]), float(c["stopping_time"]),
                                                           int(c["relax"]), float(c["speed_factor"]), float(c["accel_factor"]),
                                                           hh.fmt(c["waypoints"]), hh.fmt(c["stop_at"]), hh.fmt(c["limits"])))
    out = hh.run(exe, lines, len(chains), env=env)
    res = []
    for c, line in zip(chains, out):
        S = c["waypoints"].shape[0] - 1
        x = line.split()
        head = np.array([float(v) for v in x[:2 * S + 1]])
        count = int(x[2 * S + 1])
        n = min(count, c["capacity"])
        rows = np.array([float(v) for v in x[2 * S + 2:]])
        assert rows.size == 4 * n, (rows.size, n)
        res.append(dict(unwrapped=head[:S + 1].copy(), seg_times=head[S + 1:].copy(), count=count, rows=rows.reshape(n, 4)))
    return res


def oracle_chain(c):
    """mto_fallback_sampling through pyoracle.lib() -> (count, rows [min(count, capacity)][4])"""
    w, lim = po._f64(c["waypoints"]), po._f64(c["limits"])
    stop = np.ascontiguousarray(c["stop_at"], dtype=np.uint8)
    prm = po.default_policy(fallback_speed_factor=float(c["speed_factor"]), fallback_accel_factor=float(c["accel_factor"]),
                            fallback_stopping_time=float(c["stopping_time"]))
    out = np.zeros((c["capacity"], 4))
    n = po.lib().mto_fallback_sampling(po._dp(w), stop.ctypes.data_as(po.C.POINTER(po.C.c_uint8)), w.shape[0], po._dp(lim),
                                       int(c["relax"]), po.C.byref(prm), float(c["dt"]), po._dp(out), c["capacity"])
    return n, out[:min(n, c["capacity"])].copy()


def oracle_unwrap(waypoints):
    """the sequential unwrap of :1233-1241 through pyoracle.unwrap_heading -> the headings [V]"""
    w = np.asarray(waypoints, dtype=np.float64)
    out, last = [], float(w[0, 3])
    for v in range(w.shape[0]):
        last = po.unwrap_heading(w[v, 3], last)
        out.append(last)
    return np.array(out)


def chains(batch, seed, dt=0.2, capacity=4096, uniform=False):
    """the paths of a problem.Batch as chain problems: random stop_at, every second path with a relaxed heading, raw headings
    spread beyond [0, 2 pi) so that the unwrap has something to do; the factors and the stopping time vary from path to path
    unless uniform (one call of the library has one of each: 0.75, 0.5 and 2.0 then)"""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(batch.n_paths):
        wp, _, _ = batch.path(p)
        w = np.array(wp, dtype=np.float64)
        w[:, 3] = rng.uniform(-7.0, 13.0, size=w.shape[0])
        out.append(dict(waypoints=w, stop_at=(rng.random(w.shape[0]) < 0.3).astype(np.uint8), limits=np.array(batch.limits[p]),
                        relax=bool(p % 2), speed_factor=1.0 if p % 3 and not uniform else 0.75,
                        accel_factor=1.0 if p % 3 and not uniform else 0.5, dt=dt,
                        stopping_time=2.0 if p % 4 or uniform else 0.5, capacity=capacity))
    return out


def batch_problems(batch, seed, dt=0.2, capacity=160):
    """the paths of a problem.Batch as explicit-time problems: the oracle's Baca times of the chain, dyadic upstreams, and a
    capacity that some of the paths overrun"""
    rng = np.random.default_rng(seed + 1000)
    out = []
    for c in chains(batch, seed, dt=dt, uniform=True):
        unwrapped = np.array(c["waypoints"])
        unwrapped[:, 3] = oracle_unwrap(c["waypoints"])
        t = po.estimate_times(unwrapped, c["limits"], baca=True)
        up = bu.dyadic(rng, capacity * 4).reshape(capacity, 4)
        out.append(problem(c["waypoints"], t, dt, capacity, c["stop_at"], c["stopping_time"], up))
    return out


def pack(problems):
    """-> (seg_offsets int32 [P + 1], waypoints [sum V][4], stop_at uint8 [sum V], seg_times [sum S], upstream [P][cap][4]) of
    problems that share dt, stopping_time and capacity"""
    assert len({(p["dt"], p["stopping_time"], p["capacity"]) for p in problems}) == 1
    S = np.array([p["waypoints"].shape[0] - 1 for p in problems])
    so = np.concatenate([[0], np.cumsum(S)]).astype(np.int32)
    cap = problems[0]["capacity"]
    up = np.stack([p["upstream"] if p["upstream"] is not None else np.zeros((cap, 4)) for p in problems])
    return (so, np.concatenate([p["waypoints"] for p in problems]), np.concatenate([p["stop_at"] for p in problems]),
            np.concatenate([p["seg_times"] for p in problems]), up)


# ---- the reference's loop, as written ----------------------------------------------------------------------------------

def _wrap_range(a, lo, rng):
    r = math.fmod(a - lo, rng)
    if r < 0:
        r += rng
    return r + lo


def _radians_diff(minuend, subtrahend):
    d = _wrap_range(minuend, 0.0, TWO_PI) - _wrap_range(subtrahend, 0.0, TWO_PI)
    if d < -math.pi:
        d += TWO_PI
    elif d >= math.pi:
        d -= TWO_PI
    return d


def _interpolate_point(a, b, coeff):
    """interpolatePoint :1612-1625, the heading through mrs_lib's radians::interp"""
    p = [float(a[k]) + coeff * (float(b[k]) - float(a[k])) for k in range(3)]
    p.append(_wrap_range(float(a[3]) + coeff * _radians_diff(float(b[3]), float(a[3])), 0.0, TWO_PI))
    return p


def _c_round(x):
    """C's round() for x >= 0: halves away from zero (Python's round() goes to even)"""
    return int(math.floor(x + 0.5))


def reference_loop(p):
    """:1327-1381 push_back by push_back on explicit segment times -> dict(count, n_samples, seg_first_row [S], rows [n][4],
    row_segment [n], row_coeff [n]).  The reference has no capacity: here the loop stops pushing once the capacity is overrun
    and reports capacity + 1, the library's convention (and what keeps a time of +inf, whose ceil() Python refuses, finite:
    it stands for a count of 2^31 with the step 1.0 / inf)."""
    w, stop, dt, cap = p["waypoints"], p["stop_at"], p["dt"], p["capacity"]
    n_wp = w.shape[0]
    states, seg, coeffs, first = [], [], [], []
    count = 0
    for i in range(n_wp - 1):
        first.append(min(count, cap + 1))
        segment_time = float(p["seg_times"][i])
        n_samples, interp_step = 0, 0.0
        if segment_time > 1e-1:
            q = segment_time / dt
            n_samples = COUNT_CLAMP if math.isinf(q) else math.ceil(q)
            interp_step = 1.0 / (q if math.isinf(q) else float(n_samples)) if n_samples > 0 else 0.5
        if n_samples > 0 and i == n_wp - 2:
            n_samples += 1
        for j in range(n_samples):
            if count > cap:
                break
            point = _interpolate_point(w[i], w[i + 1], j * interp_step)
            point[3] = po.wrap_yaw(point[3])
            repeat = 1
            if j == 0 and i > 0 and stop[i]:
                repeat += _c_round(p["stopping_time"] / dt)
            for _ in range(repeat):
                if count < cap:
                    states.append(point)
                    seg.append(i)
                    coeffs.append(j * interp_step)
                count += 1
    return dict(count=count, n_samples=min(count, cap + 1), seg_first_row=np.array(first, dtype=np.int64),
                rows=np.array(states, dtype=np.float64).reshape(-1, 4), row_segment=seg, row_coeff=coeffs)


def backward_restatement(p, ref=None, reverse=False):
    """dL/dwaypoints [S + 1][4] in Python floats in the pinned order: vertex v from 0.0, the rows of segment v - 1 in
    increasing row index, each addend coeff * g rounded and then added, then the rows of segment v with (1.0 - coeff) * g.
    The row -> (segment, coeff) map is the reference loop's.  reverse: the same addends in DECREASING row index (what the
    library must not compute)."""
    ref = reference_loop(p) if ref is None else ref
    S = p["waypoints"].shape[0] - 1
    n = min(ref["count"], p["capacity"])
    up = p["upstream"]
    out = np.zeros((S + 1, 4))
    for v in range(S + 1):
        for k in range(4):
            addends = [ref["row_coeff"][r] * float(up[r, k]) for r in range(n) if ref["row_segment"][r] == v - 1]
            addends += [(1.0 - ref["row_coeff"][r]) * float(up[r, k]) for r in range(n) if ref["row_segment"][r] == v]
            acc = 0.0
            for a in (addends[::-1] if reverse else addends):
                acc = acc + a
            out[v, k] = acc
    return out


# ---- the explicit-time edge cases --------------------------------------------------------------------------------------

def _line(S, heading=None):
    """S + 1 waypoints on a gentle zigzag, headings given or a slow turn"""
    w = np.zeros((S + 1, 4))
    w[:, 0] = 1.5 * np.arange(S + 1)
    w[:, 1] = 0.7 * (np.arange(S + 1) % 3)
    w[:, 2] = 2.0 + 0.3 * (np.arange(S + 1) % 2)
    w[:, 3] = 0.4 * np.arange(S + 1) if heading is None else heading
    return w


def edge_cases():
    """the explicit-time edge cases, as problems without upstreams (capacity 400 unless the case is about it)"""
    up1 = math.nextafter(0.1, 1.0)
    c = []

    def add(name, w, t, dt=0.2, cap=400, stop=None, stopping=2.0):
        c.append(problem(w, t, dt, cap, stop, stopping, name=name))

    add("t exactly 0.1 gives no rows", _line(3), [0.7, 0.1, 0.9])
    add("t one ulp above 0.1", _line(3), [0.7, up1, 0.9])
    add("t / dt an exact integer", _line(2), [1.0, 1.5], dt=0.25)
    add("t / dt one ulp above an integer", _line(2), [math.nextafter(1.0, 2.0), math.nextafter(1.5, 2.0)], dt=0.25)
    add("negative, NaN and +inf times", _line(4), [-3.0, float("nan"), 0.9, float("inf")], cap=50)
    add("+inf in front, the rest saturated", _line(3), [float("inf"), 0.9, 0.9], cap=20)
    add("every segment at most 0.1", _line(3), [0.1, 0.05, 0.0])
    add("a last segment without rows", _line(3), [0.9, 0.9, 0.05])
    add("one segment", _line(1), [1.3])
    add("one segment without rows", _line(1), [0.1])
    add("stop_at at vertex 0 and at the last vertex", _line(3), [0.9, 0.9, 0.9], stop=[1, 0, 0, 1])
    add("stop_at at a vertex whose segment has no rows", _line(3), [0.9, 0.05, 0.9], stop=[0, 1, 0, 0])
    add("stop_at in the middle", _line(3), [0.9, 0.9, 0.9], stop=[0, 1, 1, 0])
    add("insert 0 (stopping_time / dt = 0.4)", _line(3), [0.9, 0.9, 0.9], stop=[0, 1, 1, 0], stopping=0.08)
    add("insert 3 (stopping_time / dt = 2.5)", _line(3), [0.9, 0.9, 0.9], stop=[0, 1, 1, 0], stopping=0.5)
    base = problem(_line(3), [0.9, 0.9, 0.9], 0.2, 400, [0, 1, 1, 0], 2.0)
    count = reference_loop(base)["count"]   # 5 | 10 + 5 | 10 + 5 + 1
    assert count == 36
    add("capacity equal to the count", _line(3), [0.9, 0.9, 0.9], cap=count, stop=[0, 1, 1, 0])
    add("capacity one below the count", _line(3), [0.9, 0.9, 0.9], cap=count - 1, stop=[0, 1, 1, 0])
    add("capacity inside a dwell", _line(3), [0.9, 0.9, 0.9], cap=9, stop=[0, 1, 1, 0])
    add("capacity 1", _line(3), [0.9, 0.9, 0.9], cap=1)
    w = _line(3)
    w[2] = w[1]
    add("a == b with t > 0.1", w, [0.9, 0.9, 0.9])
    add("headings across the seam", _line(3, [6.2, 0.1, 6.1, 0.3]), [0.9, 0.9, 0.9])
    add("a heading difference of exactly pi", _line(3, [0.0, math.pi, 0.0, -math.pi]), [0.9, 0.9, 0.9])
    add("negative and > 2 pi raw headings", _line(3, [-7.5, 13.0, -0.2, 9.1]), [0.9, 0.9, 0.9])
    # coeff 0.5 of (pi - 2e-12 .. pi + 1e-12) and of its mirror: interpolated yaws within 1e-12 of +-pi
    add("an interpolated yaw next to pi", _line(2, [math.pi - 2e-12, math.pi + 1e-12, math.pi - 1e-12]), [0.4, 0.4])
    add("a path of 65 segments", _line(65), 0.3 + 0.01 * (np.arange(65) % 7), stop=(np.arange(66) % 5 == 2))
    # 12 x 5 = 60 rows, then a segment of 8 that straddles rows 63 | 64
    add("rows straddle 63 | 64", _line(14), [0.9] * 12 + [1.5, 0.9], cap=400)
    # 12 x 5 = 60 rows, then a dwell of 10 behind row 60
    add("a dwell straddles 63 | 64", _line(14), [0.9] * 14, stop=[0] * 12 + [1, 0, 0], cap=400)
    return c


def wrapped_difference(got, ref):
    """wrap(got - ref) into [-pi, pi): a flip between -pi and pi is no difference"""
    d = np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    return np.abs((d + math.pi) % TWO_PI - math.pi)

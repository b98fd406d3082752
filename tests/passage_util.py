"""Shared helpers of the tests of the waypoint passage (test_passage_host.py, test_gpu_passage.py): the fixtures, the CPU
harness of csrc/mrs_tg_passage.hpp, the oracle's scan (mto_waypoint_trajectory_idxs, mto_dist_from_segment), the small shapes
built to break the kernel, the two derived gradient bounds and a float64 torch restatement with given indices."""
import ctypes as C
import functools
import os

import numpy as np

from tests import deviation_util as du
from tests import host_harness as hh

FIXTURES = os.path.join(hh.GOLDEN, "passage_cases.json")
load_cases = functools.partial(hh.load_cases, "passage_cases.json")
build_harness = functools.partial(hh.build, "passage_harness.cpp")   # (tmp_path, sanitize=False)
EPS = 2.0 ** -52
PASS = 0.1
same_bits, dyadic = du.same_bits, du.dyadic


def problem(waypoints, samples, n_samples=None, capacity=None, status=1, grad_miss=None, grad_fraction=None):
    """one path: waypoints [W][>= 3] (W may be 0), samples [rows][>= 3]; n_samples defaults to the rows given, capacity to
    max(rows, 1); grad_miss / grad_fraction [W] (the upstreams) default to zeros"""
    w = np.array(waypoints, dtype=np.float64).reshape(-1, 3 if len(waypoints) == 0 else np.shape(waypoints)[-1])[:, :3]
    s = np.array(samples, dtype=np.float64).reshape(-1, 3 if len(samples) == 0 else np.shape(samples)[-1])[:, :3]
    n = s.shape[0] if n_samples is None else int(n_samples)
    cap = max(s.shape[0], 1) if capacity is None else int(capacity)
    gm = np.zeros(len(w)) if grad_miss is None else np.asarray(grad_miss, dtype=np.float64).reshape(-1)
    gt = np.zeros(len(w)) if grad_fraction is None else np.asarray(grad_fraction, dtype=np.float64).reshape(-1)
    assert gm.size == len(w) and gt.size == len(w) and s.shape[0] >= min(n, cap)
    return dict(waypoints=w, samples=s, n_samples=n, capacity=cap, status=int(status), grad_miss=gm, grad_fraction=gt)


def rows(p):
    """how many sample rows of the path exist for the call, whatever its status: max(min(n, capacity), 0)"""
    return max(min(p["n_samples"], p["capacity"]), 0)


def run_harness(exe, problems, env=None):
    """-> per problem dict(count, index [W] int (-1 where not reached), miss [W], fraction [W], grad_samples [m][3],
    grad_waypoints [W][3], raw), m = rows(p)"""
    lines = []
    for p in problems:
        m = rows(p)
        lines.append("%d %d %d %d %s %s %s %s\n" % (len(p["waypoints"]), p["n_samples"], p["capacity"], p["status"],
                                                    hh.fmt(p["waypoints"]), hh.fmt(p["samples"][:m]), hh.fmt(p["grad_miss"]),
                                                    hh.fmt(p["grad_fraction"])))
    out = hh.run(exe, lines, len(problems), timeout=900, env=env)
    res = []
    for p, line in zip(problems, out):
        W, m = len(p["waypoints"]), rows(p)
        x = line.split()
        assert len(x) == 1 + 3 * W + 3 * m + 3 * W, (len(x), W, m)
        f = np.array([float(v) for v in x[1 + W:]])
        res.append(dict(count=int(x[0]), index=np.array([int(v) for v in x[1:1 + W]], dtype=np.int64), miss=f[:W].copy(),
                        fraction=f[W:2 * W].copy(), grad_samples=f[2 * W:2 * W + 3 * m].reshape(m, 3),
                        grad_waypoints=f[2 * W + 3 * m:].reshape(W, 3), raw=line))
    return res


# ------------------------------------------------------------------------------------------------------------------------
# the oracle's scan

_fast = {}


def _dist_by_address(po):
    if "fn" not in _fast:
        proto = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_void_p, C.c_void_p)
        _fast["fn"] = C.cast(po.lib().mto_dist_from_segment, proto)
    return _fast["fn"]


def oracle_scan_rows(po, waypoints4, samples4, n):
    """mto_waypoint_trajectory_idxs on the first n rows of samples4 [>= n][4] for waypoints4 [W][4] (contiguous float64), and
    mto_dist_from_segment of every hit -> dict(count, index [W] (-1 where not reached), miss [W] (0 where not reached))"""
    w = np.ascontiguousarray(waypoints4, dtype=np.float64).reshape(-1, 4)
    s = np.ascontiguousarray(samples4, dtype=np.float64).reshape(-1, 4)
    W = w.shape[0]
    index, miss = np.full(W, -1, dtype=np.int64), np.zeros(W)
    if W == 0 or n < 2:
        return dict(count=0, index=index, miss=miss)
    assert s.shape[0] >= n
    idx = np.zeros(W + 4, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    k = po.lib().mto_waypoint_trajectory_idxs(s.ctypes.data_as(dp), int(n), w.ctypes.data_as(dp), W,
                                              idx.ctypes.data_as(C.POINTER(C.c_int32)))
    D = _dist_by_address(po)
    for j in range(k):
        i = int(idx[j])
        index[j] = i
        miss[j] = D(w.ctypes.data + 32 * j, s.ctypes.data + 32 * i, s.ctypes.data + 32 * (i + 1))
    return dict(count=int(k), index=index, miss=miss)


def _pad4(a):
    out = np.zeros((len(a), 4))
    out[:, :3] = a
    return out


def oracle_scan(po, p):
    """oracle_scan_rows of one problem (nothing is scanned for a path with status <= 0)"""
    m = rows(p) if p["status"] > 0 else 0
    return oracle_scan_rows(po, _pad4(p["waypoints"]), _pad4(p["samples"][:m]), m)


def oracle_dist(po, p, a, b):
    f = lambda v: np.ascontiguousarray(list(v)[:3] + [0.0], dtype=np.float64)   # noqa: E731
    p4, a4, b4 = f(p), f(a), f(b)
    return float(_dist_by_address(po)(p4.ctypes.data, a4.ctypes.data, b4.ctypes.data))


# ------------------------------------------------------------------------------------------------------------------------
# shapes

STEP = 0.25


def straight(n, y=0.3, z=0.0):
    """n samples 0.25 apart along x"""
    s = np.zeros((n, 3))
    s[:, 0] = STEP * np.arange(n)
    s[:, 1] = y
    s[:, 2] = z
    return s


def on_step(i, off=0.02, y=0.3, z=0.0, at=0.5):
    """a waypoint beside step i of straight(): `off` away from it at the fraction `at` -- hit by step i and by no other step
    (the ends of its neighbours are at least 0.125 away)"""
    return [(i + at) * STEP, y + off, z]


def small_shapes():
    """name -> problem: the shapes of the issue, each built so that the property its name states holds (the host test asserts
    the properties on the oracle's scan; the GPU test compares the kernels with the harness on the same problems)"""
    rng = np.random.default_rng(20261018)
    out = {}

    def add(name, w, s, **kw):
        p = problem(w, s, **kw)
        p["grad_miss"], p["grad_fraction"] = dyadic(rng, len(p["waypoints"])), dyadic(rng, len(p["waypoints"]))
        out[name] = p

    for W in (1, 2, 5, 31):
        w = du.polyline(max(W - 1, 1), 300 + W)
        add("W%d" % W, w[:W], du.walk(w, 20 * W + 7, 0.12, W))
    w = du.polyline(4, 7)
    for n in (0, 1, 2, 63, 64, 65, 66, 129):
        add("n%d" % n, w, du.walk(w, max(n, 1), 0.08, 40 + n), n_samples=n, capacity=max(n, 2) + 3)
    add("overflow", w, du.walk(w, 70, 0.08, 9), n_samples=71, capacity=70)
    s = straight(140)
    add("hit_on_lane_63", [on_step(63), on_step(90, -0.03)], s)
    add("hit_on_lane_0_of_chunk_2", [on_step(20, 0.05), on_step(64, 0.01, at=0.625)], s)
    add("hits_on_steps_63_and_64", [on_step(10), on_step(63, 0.04, at=0.75), on_step(64, -0.02, z=0.03), on_step(100)], s)
    add("hit_on_the_last_step_of_a_full_chunk", [on_step(5), on_step(63, 0.03)], s[:65])
    add("adjacent_steps", [on_step(11), on_step(12, 0.05, at=0.125), on_step(30)], s[:40])
    add("five_hits_in_a_chunk", [on_step(8 + 9 * j, 0.01 * (j + 1), z=0.01 * j) for j in range(5)], s[:64])
    add("seventy_collinear", [on_step(i, 0.03) for i in range(70)], s[:80])
    add("never_reached_with_near_ones_behind", [on_step(5), [3.0, 5.0, 0.0], on_step(20), on_step(30)], s[:50])
    back = np.concatenate([straight(40), straight(40)[::-1] + [0.0, 0.01, 0.0]])   # out to x = 9.75 and back to 0
    add("all_reached_early_then_back_at_w0", [on_step(3), on_step(10)], back)
    nan = straight(80)
    nan[30, 1] = np.nan
    add("nan_row_passed_over", [on_step(10), on_step(50)], nan)
    add("nan_row_blocks", [on_step(10), on_step(30), on_step(50)], nan)
    dup = np.concatenate([s[:21], s[20:60]])                          # rows 20 and 21 coincide
    add("coincident_samples", [on_step(19), [20 * STEP, 0.35, 0.0], on_step(40)], dup)
    exact = straight(40, y=0.25)
    add("waypoint_on_its_step", [on_step(4, 0.0, y=0.25), on_step(9, 0.0, y=0.25, at=0.5625), on_step(20, 0.0625, y=0.25)], exact)
    add("no_waypoints", np.zeros((0, 3)), s[:30])
    # the threshold: x = 0.5, on a step along x from 0 to 1; D = |y| in bits
    unit = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    add("threshold_at_0p1_is_no_hit", [[0.5, 0.1, 0.0]], unit)
    add("threshold_below_0p1_is_a_hit", [[0.5, float(np.nextafter(0.1, 0.0)), 0.0]], unit)
    return out


def ragged_batch(n_paths, seed, lo=3, hi=30, every=1, extra=0):
    """problems on polylines of lo .. hi segments in an order that is not sorted by segment count, one with status 0 between
    good ones -> (problems, segment counts).  The requested waypoints are every `every`-th vertex of the polyline, plus `extra`
    points off the path put between them (never reached when the walk keeps away from them)"""
    rng = np.random.default_rng(seed)
    probs, S = [], []
    for q in range(n_paths):
        nseg = int(rng.integers(lo, hi + 1))
        w = du.polyline(nseg, seed * 1000 + q)
        n = int(rng.integers(9 * nseg, 14 * nseg))
        req = [x for x in w[::every]]
        for _ in range(extra):
            at = int(rng.integers(1, len(req) + 1))
            req.insert(at, req[at - 1] + rng.uniform(-0.08, 0.08, 3) * (1 if rng.integers(2) else 12))
        p = problem(np.array(req), du.walk(w, n, float(rng.uniform(0.02, 0.2)), q), capacity=14 * hi + 5)
        p["grad_miss"], p["grad_fraction"] = dyadic(rng, len(req)), dyadic(rng, len(req))
        probs.append(p)
        S.append(nseg)
    if n_paths > 2:
        probs[1]["status"] = 0
    return probs, S


# ------------------------------------------------------------------------------------------------------------------------
# the derived bounds (tests/test_passage_host.py states the derivation)

def miss_bound(p, a, b, d, g):
    """16 eps max(|p|, |a|, |b|) / d |g| per entry of the three rows of one hit (0 where it contributes exactly 0)"""
    if g == 0.0 or d == 0.0:
        return 0.0
    return 16.0 * EPS * max(np.linalg.norm(p), np.linalg.norm(a), np.linalg.norm(b)) / d * abs(g)


def fraction_bound(p, a, b, g):
    """40 eps (1 + |q| / len) / len |g| per entry of the three rows of one interior hit, q = p - a, len = |b - a|"""
    ln = np.linalg.norm(np.asarray(b) - np.asarray(a))
    if g == 0.0 or ln == 0.0:
        return 0.0
    return 40.0 * EPS * (1.0 + np.linalg.norm(np.asarray(p) - np.asarray(a)) / ln) / ln * abs(g)


# ------------------------------------------------------------------------------------------------------------------------
# float64 torch restatement, indices given

def torch_passage(torch, samples, waypoints, index, path_of_wp):
    """(miss [sum W], fraction [sum W]) of waypoints [sum W][>= 3] against samples [P][cap][>= 3] with the indices given (index
    [sum W] int, -1 = not reached: zeros) and path_of_wp [sum W] the path of every waypoint; differentiable in samples and
    waypoints, the branch chosen as distFromSegment chooses it"""
    hit = index >= 0
    i = index.clamp(min=0).to(torch.int64)
    q = path_of_wp.to(torch.int64)
    p = waypoints[..., :3]
    a, b = samples[q, i][..., :3], samples[q, torch.clamp(i + 1, max=samples.shape[1] - 1)][..., :3]
    sv = b - a
    ln = sv.norm(dim=-1)
    n = torch.where((ln > 0)[..., None], sv / ln.clamp(min=1e-300)[..., None], sv)
    coord = (n * (p - a)).sum(-1)
    foot = a + n * coord[..., None]
    before, behind = coord < 0, coord > ln
    target = torch.where(before[..., None], a, torch.where(behind[..., None], b, foot))
    diff = p - target
    d2 = (diff * diff).sum(-1)
    live = hit & (d2 > 0)
    miss = torch.where(live, torch.where(live, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
    inner = hit & ~before & ~behind & (ln > 0)
    tau = torch.where(inner, coord / torch.where(inner, ln, torch.ones_like(ln)), torch.zeros_like(ln))
    tau = torch.where(hit & behind, torch.ones_like(tau), tau)
    return miss, tau


# ------------------------------------------------------------------------------------------------------------------------
# the chain solve -> sample -> waypoint_passage -> loss (the paths, rows and step of deviation_util's chain)

CHAIN_CAPACITY = 128   # rows per path: every sample of the chain's paths fits (80 to 115 at 0.2 s)


def chain_request(batch):
    """the requested waypoints of the chain test [sum V][4]: the batch's vertices moved 2 to 5 cm off the path, each by its own
    fixed offset -- waypoints that are no vertices of the solved path, which the trajectory passes without touching"""
    req = np.array(batch.waypoints, dtype=np.float64, copy=True)
    k = np.arange(req.shape[0])
    req[:, 0] += 0.02 + 0.005 * (k % 3)
    req[:, 1] -= 0.03 - 0.004 * (k % 4)
    req[:, 2] += 0.025 * np.where(k % 2 == 0, 1.0, -1.0)
    return req

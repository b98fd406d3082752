"""The saturated-device solve kernels (mrs_tg_quad.hip) at 16 to 24 segments, every path against the oracle in 113 bits.

A launch of 6144 or more paths is solved by solve_quad_kernel, solve_duo_kernel or their group twins while the four-lane
record store fits 80 KB of LDS: up to 24 segments (22 with the records of free end vertices).  The other GPU tests of these
kernels stop at 15 segments; what runs only above that is held here:

  * the two-sided kernel's second prologue trip (segments and vertices 16 ..: times, masks, positions, the feasibility scaling);
  * launches above 64 KB of dynamic LDS (the four-lane kernels from 20 segments, their free-end instantiation from 18);
  * below-snap batches of 23 and 24 segments, whose free-end records no longer fit: every wavefront on the general step;
  * the uniform loops and the coefficient exchange through LDS with sides of 8 to 12 steps, and with S_u < Smax.

The reference is the CPU oracle in 113 bits at the segment times the HIP path used, over EVERY path.  e_h = HIP against 113 bits,
e_o = the double-precision oracle against 113 bits (tests/util.py::coeff_error, per path).  Two double-precision eliminations
in different orders differ by a modest factor of cond * eps, so the gates stand a margin of 10 over the reference's OWN error:

  1. every path: e_h <= 10 * max(e_o, P99(e_o)); relative cost error against 113 bits <= max(1e-9, 10 * e_o);
  2. median(e_h) <= 10 * median(e_o), and for plain min-snap batches the project's median(e_h) < 1e-12;
  3. statuses equal the oracle's (all 1);
  4. a path with e_o > 1e-4 is beyond double precision: finite with status 1 is all that is asked -- of at most ONE path per batch;
  5. continuity and constraint defects < 1e-9 on every 41st path and the paths of the first and the last wavefront.

Every case prints one ERR line (median / P99 / max of e_h, then of e_o, the worst e_h / max(e_o, P99(e_o)), the kernel).
NOT YET MEASURED on an MI355X: profiles/solve_16_to_24_segments.txt says what has and has not run; the first run's lines belong
there and here.  The reference's side is measured (CPU, every path; median / P99 / max of e_o):

  min-snap 16 / 17 / 20 / 24     5.9e-12   1.6 .. 2.5e-10   4.6e-8 / 4.9e-6 / 7.4e-2 (path 1134, a 0.061 s segment) / 9.4e-7
  ragged 16-24 + short paths     6.0e-12   2.1e-10          3.3e-7
  d = 2 at 18 / 22 / 23          2.4e-9    4.1 .. 4.3e-8    2.5e-7 / 2.9e-7 / 6.6e-7
  d = 3 at 22 / 24               2.4e-11   1.2 .. 1.4e-9    1.9e-6 / 6.2e-7
  mixed patterns d = 4 / d = 2   4.1e-11 / 4.8e-9   6.7e-9 / 1.2e-7   2.8e-7 / 7.7e-7
  every path in motion x 20      6.2e-12   1.7e-10          2.3e-2 (path 1134 again; the first seed tried)

so a fixed 1e-7 against the DOUBLE oracle, the gate of the tests up to 15 segments, would not hold for the reference itself.
"""
import functools

import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, problem as pr
from oracle import pyoracle as po
from tests import util

pytestmark = pytest.mark.gpu

N = 6403                    # 800 whole two-sided wavefronts + 3 paths: the last wavefront of both kernels is partly filled
BEYOND_DOUBLE = 1e-4        # gate 4
DEFECT_BOUND = 1e-9         # gate 5 (the project's bound: tests/test_gpu_round6.py)
DUO, QUAD, QUAD_ENDS = "solve_duo_kernel<false>", "solve_quad_kernel<false>", "solve_quad_kernel<false, true>"


def _ragged_with_short_paths():
    """6403 paths of 16..24 segments, the first 4800 sorted by length (runs of uniform wavefronts with S_u < Smax), the rest in
    drawn order, and six paths of one or two segments: a one-segment path puts its whole wavefront on the general step"""
    segs = [16 + pr.SplitMix64(88000 + p).next_u64() % 9 for p in range(N)]
    segs[:4800] = sorted(segs[:4800])
    for p in (4803, 5000, 5001, 6402):
        segs[p] = 1
    for p in (4900, 6401):
        segs[p] = 2
    parts = [pr.build_vertices(pr.random_box_waypoints(S, 2_400_000 + p), pr.SNAP) for p, S in enumerate(segs)]
    return pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (N, 1)))


MOVING_SEED0 = 20_000_000   # case A's 20-segment batch (oracle statuses all 1, one path beyond double precision: checked on the CPU)


def _build(key):
    kind = key[0]
    if kind == "snap":
        return pr.random_batch(N, key[1], seed0=1_000_000 * key[1])
    if kind == "ragged":
        return _ragged_with_short_paths()
    if kind == "below":
        d, S = key[1], key[2]
        return pr.random_batch(N, S, seed0=1_000_000 * S + 100_000 * d, derivative_to_optimize=d)
    if kind == "mixed":
        return pr.random_mixed_batch(N, key[1], seed0=3_300_000 + key[1], max_segments=24)
    if kind == "moving":
        from tests.test_gpu_large_batches import _moving
        return _moving(pr.random_batch(N, 20, seed0=MOVING_SEED0))
    raise KeyError(key)


def _oracles(batch, times):
    """(double-precision oracle, 113-bit oracle) of the fixed-times solve over every path"""
    args = (batch.seg_offsets, batch.waypoints, batch.fixed_mask, batch.fixed_values, batch.limits, times)
    ref_d = po.solve_batch(*args, deriv=batch.derivative_to_optimize, n_threads=16)
    po.lib().mto_set_arithmetic(po.QUAD_PRECISION)
    try:
        ref_q = po.solve_batch(*args, deriv=batch.derivative_to_optimize, n_threads=16)
    finally:
        po.lib().mto_set_arithmetic(po.REFERENCE_ARITHMETIC)
    return ref_d, ref_q


def _path_errors(c, ref, so):
    return np.array([util.coeff_error(c[a:b], ref[a:b]) for a, b in zip(so[:-1], so[1:])])


class _Reference:
    def __init__(self, batch, times):
        self.batch, self.times = batch, times
        self.ref_d, self.ref_q = _oracles(batch, times)
        self.e_o = _path_errors(self.ref_d["coeffs"], self.ref_q["coeffs"], batch.seg_offsets)
        for a in (self.times, self.e_o, self.ref_q["coeffs"], self.ref_q["cost"], self.ref_q["status"]):
            a.setflags(write=False)


@functools.lru_cache(maxsize=2)   # (the kernel variants of one batch follow each other; ~130 MB per entry)
def _reference(key):
    """The batch of `key`, the oracle's Euclidean segment times, and both oracle results at those times -- computed once"""
    batch = _build(key)
    return _Reference(batch, util.oracle_times(batch))


def _stats(e):
    return float(np.median(e)), float(np.percentile(e, 99)), float(np.max(e))


def _checked_paths(n_paths, extra=()):
    """gate 5's paths: a stride of 41, the first and the last wavefront of both kernels (16 paths cover either), and `extra`"""
    return sorted(set(range(0, n_paths, 41)) | set(range(16)) | set(range(n_paths // 16 * 16 - 16, n_paths)) | set(extra))


def _gates(name, kernel, ref, out, plain_snap, defect_paths=None, statuses=True, cap=1):
    """gates 1-5 of the module docstring on one result (out: dict of coeffs, cost, status over every path)"""
    batch, so = ref.batch, ref.batch.seg_offsets
    e_o = ref.e_o
    e_h = _path_errors(out["coeffs"], ref.ref_q["coeffs"], so)
    p99 = float(np.percentile(e_o, 99))
    floor = np.maximum(e_o, p99)
    beyond = (e_o > BEYOND_DOUBLE) if cap is not None else np.zeros(e_o.size, dtype=bool)   # (cap None: no path is exempt)
    within = ~beyond
    ratio = e_h[within] / floor[within]
    cost_err = np.abs(out["cost"] - ref.ref_q["cost"]) / np.abs(ref.ref_q["cost"])
    print("ERR %-28s %-32s e_h median %.2e P99 %.2e max %.2e | e_o median %.2e P99 %.2e max %.2e | worst e_h / max(e_o, P99) %.3g"
          " | cost %.2e | beyond double %s" % ((name, kernel) + _stats(e_h[within]) + _stats(e_o) +
                                               (float(ratio.max()), float(cost_err[within].max()), np.nonzero(beyond)[0].tolist())))
    # 3 and 4
    if statuses:
        assert np.all(ref.ref_q["status"] == 1) and np.array_equal(out["status"], ref.ref_q["status"]), \
            np.nonzero(out["status"] != ref.ref_q["status"])[0][:8]
    assert int(beyond.sum()) <= (cap or 0), np.nonzero(beyond)[0]
    assert np.all(np.isfinite(out["coeffs"])) and np.all(np.isfinite(out["cost"]))
    # 1
    worst = int(np.argmax(np.where(within, e_h / floor, 0.0)))
    assert np.all(e_h[within] <= 10.0 * floor[within]), (worst, e_h[worst], e_o[worst], p99)
    bad = within & ~(cost_err <= np.maximum(1e-9, 10.0 * e_o))
    assert not bad.any(), (np.nonzero(bad)[0][:8], cost_err[bad][:8], e_o[bad][:8])
    # 2
    assert np.median(e_h) <= 10.0 * np.median(e_o), (np.median(e_h), np.median(e_o))
    if plain_snap:
        assert np.median(e_h) < 1e-12, np.median(e_h)
    # 5
    paths = _checked_paths(batch.n_paths) if defect_paths is None else defect_paths
    paths = [p for p in paths if not beyond[p]]
    cd = util.continuity_defect(batch, out["coeffs"], ref.times, paths)
    kd = util.constraint_defect(batch, out["coeffs"], ref.times, paths)
    assert cd < DEFECT_BOUND and kd < DEFECT_BOUND, (cd, kd)


def _solve_kernels(trace):
    return [k for k in trace if k.startswith("solve_")]


def _through_solve_batch(ctx, ref, kernel, **opts):
    """mrs_tg_solve_batch (value array; it sets the constrained-slots hint itself) at ref.times; the trace names `kernel` alone"""
    api.kernel_trace_reset()
    out = ctx.solve_batch(ref.batch, ref.times, **opts)
    trace = api.kernel_trace()
    assert _solve_kernels(trace) == [kernel], trace
    assert np.array_equal(out["times"], ref.times)
    return out


def _through_bind_solve(ctx, ref, kernel, flags=0):
    """Plan.bind_solve (no hint but `flags`) at ref.times"""
    batch = ref.batch
    plan = api.Plan(ctx, batch.seg_offsets)
    db = api.DeviceBatch(batch, "cuda:0")
    db.seg_times.copy_(torch.from_numpy(ref.times))
    opt = api.default_options(derivative_to_optimize=batch.derivative_to_optimize, flags=flags)
    call = plan.bind_solve(opt, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints)
    api.kernel_trace_reset()
    call()
    trace = api.kernel_trace()
    torch.cuda.synchronize()
    out = dict(coeffs=db.coeffs.cpu().numpy(), cost=db.cost.cpu().numpy(), status=db.status.cpu().numpy())
    plan.close()
    assert _solve_kernels(trace) == [kernel], trace
    return out


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("coeffs", "cost", "status"))


def _set_duo(monkeypatch, duo):
    monkeypatch.setenv("MRS_TG_DUO", duo)       # (read at every call)
    monkeypatch.delenv("MRS_TG_DUO_UNIFORM", raising=False)


# ---- A: uniform lengths, min-snap.  16: the first length with a vertex in the second prologue trip; 17: odd, the first with
# segment index 16, side 0 one step longer than side 1; 24: the last that fits; 20: the first four-lane launch above 64 KB
# (20 last: case E below shares its reference)
@pytest.mark.parametrize("S,duo", [(S, duo) for S in (16, 17, 24, 20) for duo in ("1", "0")])
def test_uniform_min_snap(gpu_ctx, monkeypatch, S, duo):
    _set_duo(monkeypatch, duo)
    ref = _reference(("snap", S))
    kernel = DUO if duo == "1" else QUAD
    out = _through_solve_batch(gpu_ctx, ref, kernel)
    _gates("A min-snap %d" % S, kernel, ref, out, plain_snap=True)
    # the <true> instantiations: positions read from the waypoint array
    wp = _through_bind_solve(gpu_ctx, ref, kernel.replace("<false>", "<true>"), flags=api.FLAG_POSITIONS_ARE_WAYPOINTS)
    assert _same_bits(out, wp)
    if duo == "1":   # every wavefront through the predicated loops and the plain stores
        monkeypatch.setenv("MRS_TG_DUO_UNIFORM", "0")
        assert _same_bits(out, _through_solve_batch(gpu_ctx, ref, kernel))


# ---- E: the grouped dispatch at 20 segments (the four-lane group kernel above 64 KB) against the single launch of its family
@pytest.mark.parametrize("duo", [None, "0"])
def test_grouped_dispatch_of_two_at_20_segments(gpu_ctx, monkeypatch, duo):
    ref = _reference(("snap", 20))
    batch, half = ref.batch, 3200
    _set_duo(monkeypatch, "1" if duo is None else "0")
    single = _through_solve_batch(gpu_ctx, ref, DUO if duo is None else QUAD)
    if duo is None:
        monkeypatch.delenv("MRS_TG_DUO")       # the default: by wavefronts per SIMD
    plan = api.Plan(gpu_ctx, batch.seg_offsets[:half + 1])
    opt = api.default_options(derivative_to_optimize=4)
    dbs, calls = [], []
    for j in range(2):
        db = api.DeviceBatch(batch.select(range(j * half, (j + 1) * half)), "cuda:0")
        db.seg_times.copy_(torch.from_numpy(ref.times[j * half * 20:(j + 1) * half * 20]))
        calls.append(plan.bind_solve(opt, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost,
                                     waypoints=db.waypoints))
        dbs.append(db)
    api.kernel_trace_reset()
    api.RoundRobin(calls, grouped=True)(2)
    trace = api.kernel_trace()
    torch.cuda.synchronize()
    got = {k: np.concatenate([getattr(db, k).cpu().numpy() for db in dbs]) for k in ("coeffs", "cost", "status")}
    calls.clear()
    plan.close()
    assert trace == ["solve_duo_group_kernel<false>" if duo is None else "solve_quad_group_kernel<false>"], trace
    n_seg = 2 * half * 20
    assert np.array_equal(got["coeffs"], single["coeffs"][:n_seg])
    assert np.array_equal(got["cost"], single["cost"][:2 * half]) and np.array_equal(got["status"], single["status"][:2 * half])
    assert np.all(got["status"] == 1)


# ---- B: ragged 16..24 plus very short paths
@pytest.mark.parametrize("duo", ["1", "0"])
def test_ragged_16_to_24_with_very_short_paths(gpu_ctx, monkeypatch, duo):
    _set_duo(monkeypatch, duo)
    ref = _reference(("ragged",))
    batch = ref.batch
    lens = np.diff(batch.seg_offsets)
    assert lens.max() == 24 and sorted(set(lens.tolist())) == [1, 2] + list(range(16, 25))
    whole = lens[:N // 8 * 8].reshape(-1, 8)
    assert int(np.sum(np.all(whole == whole[:, :1], axis=1))) == 593        # uniform two-sided wavefronts, most with S_u < Smax
    short = np.nonzero(lens == 1)[0]
    assert short.tolist() == [4803, 5000, 5001, 6402]
    # the wavefronts (of either kernel) that a one-segment path sends to the general step are among the paths of gate 5
    general = sorted({q for p in short for q in range(p // 16 * 16, min(p // 16 * 16 + 16, N))})
    paths = _checked_paths(N, general)
    assert set(general) <= set(paths) and set(range(N // 8 * 8, N)) <= set(paths)
    kernel = DUO if duo == "1" else QUAD
    out = _through_solve_batch(gpu_ctx, ref, kernel)
    so = batch.seg_offsets
    for p in range(N // 16 * 16, N):                      # the last, partly filled wavefront wrote its paths
        assert np.all(np.any(out["coeffs"][so[p]:so[p + 1]] != 0.0, axis=(1, 2))) and out["status"][p] == 1 and out["cost"][p] > 0.0
    _gates("B ragged 16-24 + short", kernel, ref, out, plain_snap=True, defect_paths=paths)
    if duo == "1":
        monkeypatch.setenv("MRS_TG_DUO_UNIFORM", "0")
        assert _same_bits(out, _through_solve_batch(gpu_ctx, ref, kernel))


# ---- C: below snap.  The free-end records fit up to 22 segments (18: the first such launch above 64 KB); at 23 and 24 every
# wavefront of solve_quad_kernel<false> takes the general step
@pytest.mark.parametrize("d,S", [(2, 18), (2, 22), (2, 23), (3, 22), (3, 24)])
def test_below_snap(gpu_ctx, monkeypatch, d, S):
    monkeypatch.delenv("MRS_TG_DUO", raising=False)
    monkeypatch.delenv("MRS_TG_QUAD_ENDS", raising=False)
    ref = _reference(("below", d, S))
    kernel = QUAD_ENDS if S <= 22 else QUAD
    out = _through_solve_batch(gpu_ctx, ref, kernel)
    _gates("C d=%d x %d" % (d, S), kernel, ref, out, plain_snap=False)


# ---- D: mixed patterns (1..24 segments, stop_at vertices, moving starts), and every path in motion at 20 segments
@pytest.mark.parametrize("d,how", [(4, "solve_batch"), (4, "bind_solve"), (2, "solve_batch")])
def test_mixed_patterns(gpu_ctx, monkeypatch, d, how):
    monkeypatch.delenv("MRS_TG_DUO_UNIFORM", raising=False)
    ref = _reference(("mixed", d))
    lens = np.diff(ref.batch.seg_offsets)
    assert lens.min() == 1 and lens.max() == 24
    if how == "solve_batch":    # the launch shape's default; the call sets the constrained-slots hint itself
        monkeypatch.delenv("MRS_TG_DUO", raising=False)
        kernel = DUO if d == 4 else QUAD
        out = _through_solve_batch(gpu_ctx, ref, kernel)
    else:                       # no hint: the stop_at wavefronts take the two-sided kernel's general step
        monkeypatch.setenv("MRS_TG_DUO", "1")
        kernel = DUO
        out = _through_bind_solve(gpu_ctx, ref, kernel)
    _gates("D mixed d=%d %s" % (d, how), kernel, ref, out, plain_snap=False)


@pytest.mark.parametrize("duo", ["1", "0"])
def test_every_path_in_motion_at_20_segments(gpu_ctx, monkeypatch, duo):
    _set_duo(monkeypatch, duo)
    ref = _reference(("moving",))
    kernel = DUO if duo == "1" else QUAD
    out = _through_solve_batch(gpu_ctx, ref, kernel)
    _gates("D moving x 20", kernel, ref, out, plain_snap=False)
    b = ref.batch   # the moving start went into the solution
    assert np.allclose(out["coeffs"][b.seg_offsets[7], :, 1], b.fixed_values[b.vertex_range(7)[0], 1], rtol=1e-9, atol=1e-12)


# ---- F: the closing solve of a Mellinger pipeline (the scaling tail's seg_times_out / tbuf for segments >= 16)
def test_closing_solve_of_a_mellinger_pipeline_at_20_segments(gpu_ctx, monkeypatch):
    monkeypatch.delenv("MRS_TG_DUO", raising=False)
    monkeypatch.delenv("MRS_TG_DUO_UNIFORM", raising=False)
    batch = pr.random_batch(6400, 20, seed0=20_000_000)
    api.kernel_trace_reset()
    out = gpu_ctx.solve_batch(batch, None, time_alloc_method=api.TIME_ALLOC_MELLINGER)
    trace = api.kernel_trace()
    assert DUO in trace, trace
    assert np.all(np.isfinite(out["times"])) and np.all(out["times"] > 0.0)
    print("MELLINGER statuses %s" % dict(zip(*[a.tolist() for a in np.unique(out["status"], return_counts=True)])))
    # the LINEAR solve at the RETURNED times: no path dependence of the optimiser in the comparison
    ref = _Reference(batch, out["times"].copy())
    _gates("F Mellinger 6400 x 20", DUO, ref, out, plain_snap=True, statuses=False, cap=None)


# ---- G: the routing, dry
def test_routes_at_the_length_limits(gpu_ctx, monkeypatch):
    for name in ("MRS_TG_DUO", "MRS_TG_QUAD_ENDS", "MRS_TG_QUAD_MIN_PATHS"):
        monkeypatch.delenv(name, raising=False)

    def route(S, d):
        plan = api.Plan(gpu_ctx, (np.arange(6401, dtype=np.int64) * S).astype(np.int32))
        r = plan.explain(api.default_options(derivative_to_optimize=d))
        plan.close()
        return r
    assert route(24, 4) == [DUO]
    r = route(25, 4)
    assert r and not any(k.startswith("solve_quad") or k.startswith("solve_duo") for k in r), r
    assert route(22, 2) == [QUAD_ENDS]
    assert route(23, 2) == [QUAD]

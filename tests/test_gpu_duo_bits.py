"""The two-sided solve (`solve_duo_body`, mrs_tg_quad.hip) keeps its BITS.

Its plain path has two pairs of elimination loops: one for wavefronts whose eight paths are all present and of one length (no
predicate, LDS addresses walked by a per-lane stride), and the predicated pair for every other wavefront.  Both run the same
floating-point operations in the same order, and the accuracy gate of tests/test_gpu_headline_kernel.py has one path of slack,
so what is held here is equality, not a tolerance:

  * tests/golden/duo_bits_headline_slot0.npz holds the segment times, coefficients, cost and status of the first 32 paths of the
    headline's slot 0 (the set-up of tests/test_gpu_headline_kernel.py: twenty slots, two dispatches of ten), as the kernel
    computed them BEFORE the uniform loops existed (this project's own output; written by `capture()` below).  The grouped
    dispatch and one single launch over the same paths reproduce it with np.array_equal, with the positions read from the
    value array and from the waypoint array (both instantiations of both kernels);
  * a ragged batch -- 7 to 12 segments, part sorted by length (wavefronts of one length next to mixed ones), part not, the last
    wavefront partly filled -- gives the same bits with MRS_TG_DUO_UNIFORM=0 (every wavefront takes the predicated loops, the
    code as it was) and without it (uniform wavefronts take the new loops, the others fall back);
  * the same for a batch of 2 to 6 segments -- the lengths at which the coefficient exchange falls back to plain stores and the
    uniform forward loop has zero or one trip -- in which whole wavefronts and single paths start in motion (the single
    launch's moving-start lines run inside the uniform forward loop);
  * tests/golden/duo_bits_ragged_and_short.npz holds, from the same earlier build, 32 paths of the ragged batch's mixed
    wavefronts and 48 of the short batch (moving and at rest): the single launch reproduces them with the knob on and off;
  * the fixture is reproduced with MRS_TG_DUO_UNIFORM=0 as well: the predicated loops were recompiled along with the new ones.
"""
import os

import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, problem as pr

pytestmark = pytest.mark.gpu

SLOTS, PATHS, SEGMENTS, GROUP = 20, 1024, 10, 10   # tests/test_gpu_headline_kernel.py's, which are bench.py's
KEPT_PATHS = 32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "duo_bits_headline_slot0.npz")


def _headline_round(flags):
    """One round of the headline's grouped issue; returns (trace, per slot dict of host arrays, lane 0's context, closer)"""
    assert torch.cuda.is_available()
    streams = [torch.cuda.current_stream(), torch.cuda.Stream(device="cuda:0")]
    lanes, slots, calls = [], [], []
    est = api.default_options(derivative_to_optimize=4, estimate_times=1)
    lin = api.default_options(derivative_to_optimize=4, flags=flags)
    so = pr.random_batch(PATHS, SEGMENTS, seed0=0).seg_offsets
    for st in streams:
        with torch.cuda.stream(st):
            ctx = api.Context(0)
            ctx.use_torch_stream()
            lanes.append((ctx, api.Plan(ctx, so)))
    for s in range(SLOTS):
        lane = s // GROUP
        ctx, plan = lanes[lane]
        batch = pr.random_batch(PATHS, SEGMENTS, seed0=s * PATHS)
        with torch.cuda.stream(streams[lane]):
            db = api.DeviceBatch(batch, "cuda:0", sample_capacity=0)
            plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
                       limits=db.limits)
        torch.cuda.synchronize()
        db.coeffs.zero_()
        db.status.zero_()
        db.cost.zero_()
        calls.append(plan.bind_solve(lin, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost,
                                     waypoints=db.waypoints))
        slots.append((batch, db))
    torch.cuda.synchronize()
    api.kernel_trace_reset()
    api.RoundRobin(calls, grouped=True)(SLOTS)
    trace = api.kernel_trace()
    torch.cuda.synchronize()
    out = [dict(batch=b, times=db.seg_times.cpu().numpy(), coeffs=db.coeffs.cpu().numpy(), cost=db.cost.cpu().numpy(),
                status=db.status.cpu().numpy()) for b, db in slots]

    def close():
        calls.clear()
        for ctx, plan in lanes:
            plan.close()
            ctx.close()
    return trace, out, lanes[0][0], close


def _first_paths(s):
    n_seg = int(s["batch"].seg_offsets[KEPT_PATHS])
    return dict(seg_times=s["times"][:n_seg], coeffs=s["coeffs"][:n_seg], cost=s["cost"][:KEPT_PATHS], status=s["status"][:KEPT_PATHS])


def capture(path=FIXTURE):
    """Writes the fixture from the library that is loaded (run once, on the build the bits are to be held to)."""
    trace, out, _, close = _headline_round(0)
    assert trace == ["solve_duo_group_kernel<false>"] * (SLOTS // GROUP), trace
    np.savez(path, **_first_paths(out[0]))
    close()
    return path


@pytest.mark.parametrize("uniform", ["1", "0"])
@pytest.mark.parametrize("positions", ["values", "waypoints"])
def test_grouped_dispatch_and_single_launch_reproduce_the_recorded_bits(positions, uniform, monkeypatch):
    # uniform = "0": every wavefront through the predicated loops and the plain stores, which were recompiled with the rest
    monkeypatch.setenv("MRS_TG_DUO_UNIFORM", uniform)
    want = np.load(FIXTURE)
    flags = api.FLAG_POSITIONS_ARE_WAYPOINTS if positions == "waypoints" else 0
    inst = "<true>" if flags else "<false>"
    trace, out, ctx, close = _headline_round(flags)
    try:
        assert trace == ["solve_duo_group_kernel" + inst] * (SLOTS // GROUP), trace
        got = _first_paths(out[0])
        # (the times are the device estimator's: held too, so that a change there is not read as a change of the solve)
        assert np.array_equal(got["seg_times"], want["seg_times"])
        for name in ("coeffs", "cost", "status"):
            assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), name
        # one launch of the single-batch kernel over the ten slots of lane 0
        parts = []
        for s in out[:GROUP]:
            b = s["batch"]
            parts += [b.path(p) for p in range(b.n_paths)]
        big = pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (len(parts), 1)))
        t = np.concatenate([s["times"] for s in out[:GROUP]])
        plan = api.Plan(ctx, big.seg_offsets)
        db = api.DeviceBatch(big, "cuda:0", sample_capacity=0)
        db.seg_times.copy_(torch.from_numpy(t))
        opt = api.default_options(derivative_to_optimize=4, flags=flags)
        api.kernel_trace_reset()
        plan.bind_solve(opt, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints)()
        assert api.kernel_trace()[-1] == "solve_duo_kernel" + inst, api.kernel_trace()
        torch.cuda.synchronize()
        one = dict(coeffs=db.coeffs.cpu().numpy(), cost=db.cost.cpu().numpy(), status=db.status.cpu().numpy())
        plan.close()
        n_seg = want["coeffs"].shape[0]
        assert np.array_equal(one["coeffs"][:n_seg], want["coeffs"])
        assert np.array_equal(one["cost"][:KEPT_PATHS], want["cost"])
        assert np.array_equal(one["status"][:KEPT_PATHS], want["status"])
        # ... and over ALL its paths the single launch is the grouped dispatch
        assert np.array_equal(one["coeffs"], np.concatenate([s["coeffs"] for s in out[:GROUP]]))
        assert np.array_equal(one["cost"], np.concatenate([s["cost"] for s in out[:GROUP]]))
    finally:
        close()


def _ragged_batch():
    """6403 paths of 7..12 segments: the first 4800 sorted by length (runs of 800 = 100 wavefronts of one length each), the
    rest in drawn order (most wavefronts mixed); 6403 = 800 wavefronts + 3 paths"""
    n = 6403
    segs = [7 + (pr.SplitMix64(77000 + p).next_u64() % 6) for p in range(n)]
    segs[:4800] = sorted(segs[:4800])
    parts = [pr.build_vertices(pr.random_box_waypoints(S, 52000 + p), pr.SNAP) for p, S in enumerate(segs)]
    return pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (n, 1)))


def _short_batch():
    """6400 paths of 2..6 segments, sorted by length: 160 uniform wavefronts per length -- the lengths at which the coefficient
    exchange has too few consumed records (S < 5: never; S = 5, 6: not in a side's first step) and the uniform forward loop has
    zero or one trip.  Some paths START IN MOTION (velocity, acceleration, jerk given at the first vertex): whole wavefronts of
    them and single ones among paths at rest.  Returns (batch, moving[path])."""
    n = 6400
    parts, moving = [], []
    for p in range(n):
        S = 2 + p // 1280
        mv = (p // 8) % 5 == 0 or p % 41 == 0
        rng = pr.SplitMix64(91000 + p)
        state = dict(heading=rng.uniform(-3.0, 3.0), velocity=[rng.uniform(-2.0, 2.0) for _ in range(4)],
                     acceleration=[rng.uniform(-1.0, 1.0) for _ in range(4)], jerk=[rng.uniform(-1.0, 1.0) for _ in range(4)])
        parts.append(pr.build_vertices(pr.random_box_waypoints(S, 63000 + p), pr.SNAP, initial_state=state if mv else None))
        moving.append(mv)
    return pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (n, 1))), np.array(moving)


def _solve_with_and_without_the_knob(gpu_ctx, monkeypatch, batch, at_rest):
    """{(positions, knob): (single launch (coeffs, cost, status), grouped dispatch's coeffs)}; the grouped dispatch (compiled
    without the moving-start lines: such paths take its general step) is held to the single launch on the wavefronts at rest"""
    # (a wavefront of the grouped dispatch with ONE path in motion takes the general step with all eight)
    pad = np.concatenate([at_rest, np.ones(-len(at_rest) % 8, dtype=bool)]).reshape(-1, 8)
    at_rest = np.repeat(pad.all(axis=1), 8)[:len(at_rest)]
    seg_at_rest = np.repeat(at_rest, np.diff(batch.seg_offsets))
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    db = api.DeviceBatch(batch, "cuda:0")
    est = api.default_options(derivative_to_optimize=4, estimate_times=1)
    plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
               limits=db.limits)
    torch.cuda.synchronize()
    got = {}
    for positions, flags in (("values", 0), ("waypoints", api.FLAG_POSITIONS_ARE_WAYPOINTS)):
        opt = api.default_options(derivative_to_optimize=4, flags=flags)
        for uniform in ("0", "1"):
            monkeypatch.setenv("MRS_TG_DUO_UNIFORM", uniform)
            c2 = torch.zeros_like(db.coeffs)
            for t in (db.coeffs, db.status, db.cost):
                t.zero_()
            # single launch
            api.kernel_trace_reset()
            plan.bind_solve(opt, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints)()
            assert api.kernel_trace()[-1] == "solve_duo_kernel<%s>" % ("true" if flags else "false"), api.kernel_trace()
            torch.cuda.synchronize()
            single = (db.coeffs.cpu().numpy().copy(), db.cost.cpu().numpy().copy(), db.status.cpu().numpy().copy())
            # grouped dispatch of two
            db.coeffs.zero_()
            calls = [plan.bind_solve(opt, db.fixed_mask, db.fixed_values, db.seg_times, cc, db.status, db.cost, waypoints=db.waypoints)
                     for cc in (db.coeffs, c2)]
            api.kernel_trace_reset()
            api.RoundRobin(calls, grouped=True)(2)
            assert api.kernel_trace() == ["solve_duo_group_kernel<%s>" % ("true" if flags else "false")], api.kernel_trace()
            torch.cuda.synchronize()
            grouped = db.coeffs.cpu().numpy().copy()
            assert np.array_equal(grouped, c2.cpu().numpy())
            assert np.array_equal(grouped[seg_at_rest], single[0][seg_at_rest])
            assert np.array_equal(db.cost.cpu().numpy()[at_rest], single[1][at_rest])
            got[positions, uniform] = (single, grouped)
    got["seg_times"] = db.seg_times.cpu().numpy()
    plan.close()
    return got


FIXTURE_KNOB_BATCHES = os.path.join(os.path.dirname(FIXTURE), "duo_bits_ragged_and_short.npz")
RAGGED_KEPT = list(range(6000, 6032))                                                 # drawn order: mixed wavefronts
SHORT_KEPT = list(range(0, 16)) + list(range(2560, 2576)) + list(range(5120, 5136))   # 2, 4, 6 segments; moving and at rest


def _kept(batch, seg_times, single, paths, prefix):
    so = batch.seg_offsets
    segs = np.concatenate([np.arange(so[p], so[p + 1]) for p in paths])
    return {prefix + "seg_times": seg_times[segs], prefix + "coeffs": single[0][segs], prefix + "cost": single[1][paths],
            prefix + "status": single[2][paths]}


def _single_launch(ctx, batch):
    plan = api.Plan(ctx, batch.seg_offsets)
    db = api.DeviceBatch(batch, "cuda:0")
    est = api.default_options(derivative_to_optimize=4, estimate_times=1)
    plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
               limits=db.limits)
    torch.cuda.synchronize()
    for t in (db.coeffs, db.status, db.cost):
        t.zero_()
    api.kernel_trace_reset()
    plan.bind_solve(api.default_options(derivative_to_optimize=4), db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status,
                    db.cost, waypoints=db.waypoints)()
    assert api.kernel_trace()[-1] == "solve_duo_kernel<false>", api.kernel_trace()
    torch.cuda.synchronize()
    out = db.seg_times.cpu().numpy(), (db.coeffs.cpu().numpy(), db.cost.cpu().numpy(), db.status.cpu().numpy())
    plan.close()
    return out


def capture_knob_batches(path=FIXTURE_KNOB_BATCHES):
    """Writes the second fixture from the library that is loaded: the kept paths of the ragged and of the short batch"""
    ctx = api.Context(0)
    ctx.use_torch_stream()
    rag, (short, _) = _ragged_batch(), _short_batch()
    t_r, s_r = _single_launch(ctx, rag)
    t_s, s_s = _single_launch(ctx, short)
    np.savez(path, **_kept(rag, t_r, s_r, RAGGED_KEPT, "ragged_"), **_kept(short, t_s, s_s, SHORT_KEPT, "short_"))
    ctx.close()
    return path


def _assert_recorded(batch, got, seg_times, paths, prefix):
    """the single launch's kept paths against what the kernel computed before the uniform loops existed (mixed wavefronts and
    short ones are not in the headline's fixture)"""
    want = np.load(FIXTURE_KNOB_BATCHES)
    for key in (("values", "0"), ("values", "1")):
        have = _kept(batch, seg_times, got[key][0], paths, prefix)
        for name, arr in have.items():
            assert arr.shape == want[name].shape and np.array_equal(arr, want[name]), (key, name)


def _assert_one_answer(got):
    first = got["values", "0"]
    assert np.all(first[0][2] == 1)
    for key in (("values", "1"), ("waypoints", "0"), ("waypoints", "1")):
        for a, b in zip(first[0], got[key][0]):
            assert np.array_equal(a, b), key
        assert np.array_equal(first[1], got[key][1]), key


def test_ragged_batch_same_bits_through_uniform_loops_with_fallback_and_predicated_loops(gpu_ctx, monkeypatch):
    batch = _ragged_batch()
    lens = np.diff(batch.seg_offsets)
    assert lens.min() == 7 and lens.max() == 12 and batch.n_paths % 8 != 0
    whole = lens[:batch.n_paths // 8 * 8].reshape(-1, 8)
    n_uniform = int(np.sum(np.all(whole == whole[:, :1], axis=1)))
    assert 400 < n_uniform < whole.shape[0] - 100   # both kinds of wavefront in numbers
    got = _solve_with_and_without_the_knob(gpu_ctx, monkeypatch, batch, np.ones(batch.n_paths, dtype=bool))
    assert np.all(got["values", "1"][0][0][batch.seg_offsets[-1] - 1] != 0.0)   # the last, partly filled wavefront wrote its paths
    _assert_one_answer(got)
    _assert_recorded(batch, got, got["seg_times"], RAGGED_KEPT, "ragged_")


def test_short_uniform_wavefronts_and_moving_starts_same_bits_with_and_without_the_knob(gpu_ctx, monkeypatch):
    batch, moving = _short_batch()
    assert 1000 < moving.sum() < 2000
    got = _solve_with_and_without_the_knob(gpu_ctx, monkeypatch, batch, ~moving)
    _assert_one_answer(got)
    _assert_recorded(batch, got, got["seg_times"], SHORT_KEPT, "short_")
    # the moving starts went into the solution: a path in motion leaves its first vertex with the given velocity
    c = got["values", "1"][0][0]
    p = int(np.nonzero(moving)[0][0])
    v0 = batch.vertex_range(p)[0]
    assert np.allclose(c[batch.seg_offsets[p], :, 1], batch.fixed_values[v0, 1], rtol=1e-9, atol=1e-12)

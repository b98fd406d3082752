"""The two-sided solve's coefficient stores: same bytes at the same places on every store road.

`solve_duo_body` (mrs_tg_quad.hip) has three roads for a segment's 320 bytes of coefficients:

  * separate 16-byte pieces, ordinary stores: wavefronts that are not uniform (mixed lengths, the partly filled last one), the
    one step of 2 segments and step 0 of 3 segments, and everything under MRS_TG_DUO_UNIFORM=0;
  * through the LDS exchange, 64 consecutive bytes per segment and instruction, ordinary stores: uniform wavefronts of the single
    launch, and of the grouped dispatch under MRS_TG_DUO_STORE_THROUGH=0;
  * the same as write-through stores: uniform wavefronts of the grouped dispatch (the default).

The exchange buffer lies in record rows the backward loop has finished with, its sixteenth chunk in a place of its own, and the
step that only side 0 takes (odd lengths) packs eight chunks into two rows.  What can go wrong is an address, in LDS or in
memory -- a row too early (records overwritten before they are read: wrong values), a chunk or a segment off by one (right values
at the wrong place) -- so every case here

  * compares coeffs, cost and status with np.array_equal between MRS_TG_DUO_STORE_THROUGH=1 and =0 and against
    MRS_TG_DUO_UNIFORM=0 (the predicated loops and separate pieces: the road tests/test_gpu_duo_bits.py holds to recorded bits);
  * fills every output buffer with a NaN bit pattern first, inside a larger allocation with guard zones of at least one path's
    bytes on both sides: afterwards the guards are untouched and no pattern word is left inside;
  * asserts the kernel by trace.

Shapes: 8 batches of 777 paths as one grouped dispatch (6216 paths: above the two-sided kernels' lower bound of 6144, and 777 = 97
wavefronts + 1 path, so the last wavefront of every batch is partial and stores ordinary pieces next to written-through lines)
at uniform lengths 2 and 3 (no exchange but the odd length's middle step), 4 and 5 (the first step of a side is nearly the only
one), 9 and 11 (a step that only side 0 takes), 10 (the headline's), 24 (the longest routed), and a ragged batch of 2 to 12
segments; positions from the value array and from the waypoint array; and one single launch of 6403 paths of mixed lengths in
which whole wavefronts and single paths start in motion.
"""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, problem as pr

pytestmark = pytest.mark.gpu

GROUP, PATHS = 8, 777
PATTERN64 = 0x7FF8DEADBEEF5A5A   # a quiet NaN no solve produces
PATTERN32 = 0x7FC0DEAD           # (status: a float NaN's bits, no status value)
ROADS = (("1", "1"), ("0", "1"), ("1", "0"))   # (MRS_TG_DUO_STORE_THROUGH, MRS_TG_DUO_UNIFORM); the last is the reference road


class Guarded:
    """n elements inside an allocation of guard + n + guard, every word set to the pattern"""

    def __init__(self, shape, dtype, guard):
        n = int(np.prod(shape))
        self.n, self.guard = n, guard
        self.bits = torch.int64 if dtype == torch.float64 else torch.int32
        self.pattern = PATTERN64 if dtype == torch.float64 else PATTERN32
        self.whole = torch.empty(guard + n + guard, dtype=dtype, device="cuda:0")
        self.view = self.whole[guard:guard + n].view(*shape)
        self.fill()

    def fill(self):
        self.whole.view(self.bits).fill_(self.pattern)

    def checked(self, what):
        """the inside as a host array, after: guards untouched, no pattern word left inside"""
        raw = self.whole.view(self.bits).cpu().numpy()
        g, n = self.guard, self.n
        assert np.all(raw[:g] == self.pattern), what + ": written in front of the buffer"
        assert np.all(raw[g + n:] == self.pattern), what + ": written behind the buffer"
        left = np.nonzero(raw[g:g + n] == self.pattern)[0]
        assert left.size == 0, "%s: %d words not written, the first at %d" % (what, left.size, left[0])
        return self.view.cpu().numpy().copy()


def _uniform_batch(S, n=PATHS, seed=0):
    return pr.random_batch(n, S, seed0=seed + 1000 * S)


def _ragged_batch(n=PATHS):
    """2 to 12 segments: the first 616 paths sorted by length (runs of about 56 = seven uniform wavefronts per length and a
    mixed one where two runs meet), the rest in drawn order (mixed wavefronts)"""
    segs = [2 + int(pr.SplitMix64(41000 + p).next_u64() % 11) for p in range(n)]
    segs[:616] = sorted(segs[:616])
    parts = [pr.build_vertices(pr.random_box_waypoints(S, 42000 + p), pr.SNAP) for p, S in enumerate(segs)]
    return pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (n, 1)))


def _estimated(ctx, batch):
    plan = api.Plan(ctx, batch.seg_offsets)
    db = api.DeviceBatch(batch, "cuda:0")
    est = api.default_options(derivative_to_optimize=4, estimate_times=1)
    plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
               limits=db.limits)
    torch.cuda.synchronize()
    return plan, db


def _outputs(batch, count):
    lens = np.diff(batch.seg_offsets)
    g_coeff = int(lens.max()) * pr.N_DIM * pr.N_COEFF   # the longest path's coefficients
    return [(Guarded((batch.n_segments, pr.N_DIM, pr.N_COEFF), torch.float64, g_coeff),
             Guarded((batch.n_paths,), torch.float64, 64), Guarded((batch.n_paths,), torch.int32, 64)) for _ in range(count)]


def _same(got, what):
    want = got[ROADS[-1]]
    assert all(np.all(np.isfinite(c)) and np.all(np.isfinite(co)) for c, co, _ in want), what
    for road in ROADS[:-1]:
        for j, (a, b) in enumerate(zip(got[road], want)):
            for name, x, y in zip(("coeffs", "cost", "status"), a, b):
                assert np.array_equal(x, y), (what, road, j, name)


def _grouped_case(gpu_ctx, monkeypatch, batch, what):
    lens = np.diff(batch.seg_offsets)
    assert GROUP * batch.n_paths >= 6144 and batch.n_paths % 8 != 0
    plan, db = _estimated(gpu_ctx, batch)
    # eight batches of one plan: the same constraints at eight sets of times, eight sets of outputs
    times = [db.seg_times * (1.0 + 0.03 * j) for j in range(GROUP)]
    outs = _outputs(batch, GROUP)
    try:
        for positions, flags in (("values", 0), ("waypoints", api.FLAG_POSITIONS_ARE_WAYPOINTS)):
            opt = api.default_options(derivative_to_optimize=4, flags=flags)
            calls = [plan.bind_solve(opt, db.fixed_mask, db.fixed_values, t, c.view, st.view, co.view, waypoints=db.waypoints)
                     for t, (c, co, st) in zip(times, outs)]
            got = {}
            for road in ROADS:
                monkeypatch.setenv("MRS_TG_DUO_STORE_THROUGH", road[0])
                monkeypatch.setenv("MRS_TG_DUO_UNIFORM", road[1])
                for o in outs:
                    for buf in o:
                        buf.fill()
                torch.cuda.synchronize()
                api.kernel_trace_reset()
                api.RoundRobin(calls, grouped=True)(GROUP)
                assert api.kernel_trace() == ["solve_duo_group_kernel<%s>" % ("true" if flags else "false")], api.kernel_trace()
                torch.cuda.synchronize()
                got[road] = [tuple(buf.checked("%s, %s, road %s, batch %d, %s" % (what, positions, road, j, name))
                                   for buf, name in zip(o, ("coeffs", "cost", "status"))) for j, o in enumerate(outs)]
            _same(got, (what, positions))
            # (the eight batches were solved at different times: an answer written to another batch's buffer would show)
            c0, c1 = got[ROADS[0]][0][0], got[ROADS[0]][1][0]
            assert not np.array_equal(c0, c1)
            assert np.all(c0[batch.seg_offsets[-1] - 1] != 0.0) and lens.min() >= 2
    finally:
        plan.close()


@pytest.mark.parametrize("segments", [2, 3, 4, 5, 9, 10, 11, 24])
def test_grouped_dispatch_of_one_length_same_bytes_on_every_store_road(gpu_ctx, monkeypatch, segments):
    _grouped_case(gpu_ctx, monkeypatch, _uniform_batch(segments), "%d segments" % segments)


def test_grouped_dispatch_of_ragged_batches_same_bytes_on_every_store_road(gpu_ctx, monkeypatch):
    batch = _ragged_batch()
    lens = np.diff(batch.seg_offsets)
    assert lens.min() == 2 and lens.max() == 12
    whole = lens[:batch.n_paths // 8 * 8].reshape(-1, 8)
    uniform = np.all(whole == whole[:, :1], axis=1)
    assert set(whole[uniform, 0]) == set(range(2, 13)) and 20 < (~uniform).sum()   # uniform wavefronts of every length, and mixed ones
    _grouped_case(gpu_ctx, monkeypatch, batch, "ragged")


def _moving_batch():
    """6403 paths (800 wavefronts + 3 paths) of 3, 4, 5, 9, 10 and 24 segments, sorted by length; whole wavefronts and single
    paths START IN MOTION (the single launch's moving-start lines).  Returns (batch, moving[path])."""
    n, lengths = 6403, (3, 4, 5, 9, 10, 24)
    parts, moving = [], []
    for p in range(n):
        S = lengths[min(p // 1067, len(lengths) - 1)]   # (1067 = 133 wavefronts + 3 paths: mixed wavefronts where two lengths meet)
        mv = (p // 8) % 5 == 0 or p % 41 == 0
        rng = pr.SplitMix64(93000 + p)
        state = dict(heading=rng.uniform(-3.0, 3.0), velocity=[rng.uniform(-2.0, 2.0) for _ in range(4)],
                     acceleration=[rng.uniform(-1.0, 1.0) for _ in range(4)], jerk=[rng.uniform(-1.0, 1.0) for _ in range(4)])
        parts.append(pr.build_vertices(pr.random_box_waypoints(S, 94000 + p), pr.SNAP, initial_state=state if mv else None))
        moving.append(mv)
    return pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (n, 1))), np.array(moving)


def test_single_launch_with_moving_starts_same_bytes_on_every_store_road(gpu_ctx, monkeypatch):
    batch, moving = _moving_batch()
    assert 1000 < moving.sum() < 2000 and batch.n_paths % 8 != 0
    plan, db = _estimated(gpu_ctx, batch)
    (c, co, st), = _outputs(batch, 1)
    try:
        for positions, flags in (("values", 0), ("waypoints", api.FLAG_POSITIONS_ARE_WAYPOINTS)):
            opt = api.default_options(derivative_to_optimize=4, flags=flags)
            call = plan.bind_solve(opt, db.fixed_mask, db.fixed_values, db.seg_times, c.view, st.view, co.view, waypoints=db.waypoints)
            got = {}
            for road in ROADS:
                monkeypatch.setenv("MRS_TG_DUO_STORE_THROUGH", road[0])
                monkeypatch.setenv("MRS_TG_DUO_UNIFORM", road[1])
                for buf in (c, co, st):
                    buf.fill()
                torch.cuda.synchronize()
                api.kernel_trace_reset()
                call()
                assert api.kernel_trace()[-1] == "solve_duo_kernel<%s>" % ("true" if flags else "false"), api.kernel_trace()
                torch.cuda.synchronize()
                got[road] = [tuple(buf.checked("single launch, %s, road %s, %s" % (positions, road, name))
                                   for buf, name in zip((c, co, st), ("coeffs", "cost", "status")))]
            _same(got, ("single launch", positions))
            # the moving starts went into the solution: a path in motion leaves its first vertex with the given velocity
            coeffs = got[ROADS[0]][0][0]
            p = int(np.nonzero(moving)[0][0])
            v0 = batch.vertex_range(p)[0]
            assert np.allclose(coeffs[batch.seg_offsets[p], :, 1], batch.fixed_values[v0, 1], rtol=1e-9, atol=1e-12)
    finally:
        plan.close()

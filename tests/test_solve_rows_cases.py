"""The cases of tests/solve_rows_util.py, without a GPU: the reference side of test_gpu_solve_rows_lengths.py holds on every
batch (the oracle solves every path, in double and in 113 bits, and no path is beyond double precision: NO path is excused
on the GPU), and the batches reach the edges of solve_rows_kernel's schedule they are there for, by the host statement of
that schedule (so that an edit of a batch, or of the kernel's schedule, cannot lose an edge unnoticed)."""
import numpy as np
import pytest

from tests import solve_rows_util as u

BEYOND_DOUBLE = 1e-4


@pytest.mark.parametrize("key", u.ALL_KEYS, ids=u.key_id)
def test_the_oracle_solves_every_path_within_double_precision(key):
    """a condition of the GPU test, not a tolerance: a seed that breaks it is replaced (solve_rows_util._seed0)"""
    ref = u.reference(key)
    assert np.all(ref.ref_d["status"] == 1), np.nonzero(ref.ref_d["status"] != 1)[0]
    assert np.all(ref.ref_q["status"] == 1), np.nonzero(ref.ref_q["status"] != 1)[0]
    assert np.all(np.isfinite(ref.e_o)) and ref.e_o.max() <= BEYOND_DOUBLE, (int(np.argmax(ref.e_o)), ref.e_o.max())
    assert np.all(ref.times > 0.0)
    print("E_O %-28s %3d paths, e_o median %.2e P99 %.2e max %.2e" % ((u.key_id(key), ref.batch.n_paths) + u.stats(ref.e_o)))


def test_the_batches_have_their_lengths_and_patterns():
    for key in u.EVERY_KEYS[:9]:
        lens = np.diff(u.build(key).seg_offsets)
        assert lens.tolist() == [S for S in range(1, 41) for _ in range(3)]
    for key in u.EVERY_KEYS[9:]:
        lens = np.diff(u.build(key).seg_offsets)
        assert lens.size == 240 and lens.min() == 1 and lens.max() == 40
    for key in u.EDGE_KEYS + u.TAIL_KEYS:
        b = u.build(key)
        assert np.diff(b.seg_offsets).tolist() == [S for S in key[1] for _ in range(3)] and 6 <= b.n_paths <= 12
    # the patterns: a moving start constrains velocity, acceleration and jerk to non-zero values; stop_at every third interior vertex
    b = u.build(("every", 2, "moving"))
    v0 = b.vertex_range(7)[0]
    assert b.fixed_mask[v0].tolist() == [1, 1, 1, 1, 0] and np.all(b.fixed_values[v0, 1:4, :3] != 0.0)
    b = u.build(("every", 4, "stop"))
    _, m, _ = b.path(3 * 9)      # 10 segments
    assert [i for i in range(1, 10) if m[i, 1:4].all()] == [3, 6, 9] and not m[1:10, 4].any()
    mixed = u.build(("mixed", 4))
    interior_stops = sum(int(mixed.path(p)[1][1:-1, 1:4].all(axis=1).sum()) for p in range(mixed.n_paths))
    moving = sum(bool(np.any(mixed.path(p)[2][0, 1:4] != 0.0)) for p in range(mixed.n_paths))
    assert interior_stops > 100 and 60 < moving < 180


def test_the_schedule_of_the_patterns():
    fixed, free_snap, free_two = [1, 1, 1, 1, 1], [1, 1, 1, 1, 0], [1, 1, 1, 0, 0]
    assert u.schedule(1, fixed, fixed) == (0, 0, 0)
    assert u.schedule(1, free_two, free_two) == (0, 0, 1)
    assert u.schedule(2, fixed, fixed) == (1, 0, 0)
    # every arm of both switches with a refill is first reached at wmax = 8, the second trip round the quads at 12
    assert u.schedule(18, fixed, fixed) == (9, 8, 8) and u.schedule(17, fixed, fixed) == (8, 7, 8)
    assert u.schedule(26, fixed, fixed) == (13, 12, 12)
    assert u.schedule(16, free_snap, free_snap) == (8, 8, 8) and u.schedule(24, free_two, free_two) == (12, 12, 12)
    # a moving start changes nothing: at min-snap its slots 1..4 are constrained as before, below snap one stays free
    for d, kind in ((4, "rest"), (4, "moving"), (2, "rest"), (2, "moving")):
        b = u.build(("every", d, kind))
        for p in range(b.n_paths):
            S = int(b.seg_offsets[p + 1] - b.seg_offsets[p])
            mid = S // 2
            want = (mid, max(mid - 1, 0), max(S - mid - 1, 0)) if d == 4 else (mid, mid, S - mid)
            assert u.path_schedule(b, p) == want, (d, kind, p)
    assert [u.first_built(2, q) for q in range(4)] == [0, 1, 2, -1]
    assert [u.first_built(9, q) for q in range(4)] == [8, 9, 6, 7]
    assert [u.first_built(0, q) for q in range(4)] == [0, -1, -1, -1]


def test_the_every_length_batches_reach_the_schedules_edges():
    wmax_seen = {1: set(), 2: set()}
    uneven = short_sides = 0
    for key in u.EVERY_KEYS:
        b = u.build(key)
        lens = np.diff(b.seg_offsets)
        assert {1, 2} <= set(lens.tolist())
        for p in range(b.n_paths):
            _, n0, n1 = u.path_schedule(b, p)
            uneven += n0 != n1
            short_sides += sum(n < 4 and u.first_built(n, 0) == 0 for n in (n0, n1))
        for ppw in (1, 2):
            waves = u.wavefronts(b, ppw)
            assert len(waves) == (b.n_paths + ppw - 1) // ppw and [p for w in waves for p in w[0]] == u.plan_order(b.seg_offsets).tolist()
            wmax_seen[ppw] |= {w[1] for w in waves}
    assert wmax_seen[1] == set(range(21)) and wmax_seen[2] == set(range(21))
    assert uneven > 100 and short_sides > 100


@pytest.mark.parametrize("key", u.EVERY_KEYS[:9], ids=u.key_id)
def test_two_paths_per_wavefront_pairs_neighbouring_lengths(key):
    """three paths per length: at two paths per wavefront every even length shares a wavefront with the odd length below it.
    Their longer sides are equal, their shorter sides are not: the odd path's first row stops one step before wmax (its last
    step predicated off), next to wavefronts of two equal paths"""
    b = u.build(key)
    lens = np.diff(b.seg_offsets)
    assert not np.array_equal(u.plan_order(b.seg_offsets), np.arange(b.n_paths))   # the plan's order is not the caller's
    waves = u.wavefronts(b, 2)
    mixed = [w for w in waves if lens[w[0][0]] != lens[w[0][1]]]
    equal = [w for w in waves if lens[w[0][0]] == lens[w[0][1]]]
    assert len(mixed) == 20 and len(equal) == 40
    for (a, c), wmax in mixed:
        assert lens[a] == lens[c] + 1 and lens[a] % 2 == 0                           # longer first is what the order gives
        (_, a0, a1), (_, c0, c1) = u.path_schedule(b, a), u.path_schedule(b, c)
        assert a0 == a1 == c1 == wmax and c0 == max(wmax - 1, 0)
    assert all(wm == max(u.path_schedule(b, p)[1:][i] for p in ps for i in (0, 1)) for ps, wm in waves)


def test_two_paths_of_a_wavefront_with_different_wmax():
    """Under the adapter's patterns nact follows from S and the objective's order alone, and the plan puts the longer path
    first: the second path of a wavefront never has the larger wmax.  The larger one first, by one step and by many, and equal
    ones: the mixed batches (drawn lengths) and the size-edge batches (a 39-segment path next to one of 17)"""
    own = lambda b, p: max(u.path_schedule(b, p)[1:])
    gaps = set()
    for key in u.EVERY_KEYS[9:] + u.EDGE_KEYS:
        b = u.build(key)
        for ps, wmax in u.wavefronts(b, 2):
            if len(ps) == 2:
                assert own(b, ps[0]) == wmax >= own(b, ps[1])
                gaps.add(wmax - own(b, ps[1]))
    assert {0, 1} <= gaps and max(gaps) >= 25


def test_a_wavefront_with_a_single_path():
    """an odd path count leaves the last wavefront of a two-per-wavefront launch with one path (store_ok = false on its spare
    rows); the mixed batches' 240 paths fill every wavefront"""
    for key in u.EDGE_KEYS:
        b = u.build(key)
        waves = u.wavefronts(b, 2)
        if b.n_paths % 2:
            assert len(waves[-1][0]) == 1 and waves[-1][1] == max(u.path_schedule(b, waves[-1][0][0])[1:])
    assert sum(u.build(key).n_paths % 2 for key in u.EDGE_KEYS) >= 18
    # the shortest path of a size-edge batch sits in the layout of the longest: its records are Smax's strides apart
    for key in u.EDGE_KEYS:
        lens = np.diff(u.build(key).seg_offsets)
        assert lens.min() <= 7 and lens.max() >= 39


def test_the_size_rules_change_where_the_batches_stand():
    """rows_lds_bytes against the 144 KB budget and the 64 KB default limit: a path costs 102 S + 88 doubles, rounded up to even
    (it is even for every S: the rounding term is zero throughout), plus 2"""
    assert all(u.path_doubles(S) == 102 * S + 90 for S in range(1, 257))

    def last_fit(ppw, sampling, limit):
        fits = [S for S in range(1, 257) if u.lds_bytes(S, ppw, sampling) <= limit]
        assert fits == list(range(1, fits[-1] + 1))
        return fits[-1]
    assert last_fit(1, False, u.LDS_BUDGET) == 179      # the kernel applies at all
    assert last_fit(2, False, u.LDS_BUDGET) == 89       # two paths per wavefront
    assert last_fit(1, True, u.LDS_BUDGET) == 126       # sampling in the kernel's tail
    assert last_fit(1, False, u.LDS_DEFAULT) == 79      # below the default limit of a launch
    assert last_fit(2, False, u.LDS_DEFAULT) == 39
    assert last_fit(1, True, u.LDS_DEFAULT) == 54
    edges = {max(lengths) for lengths in u.SIZE_EDGE_LENGTHS}
    assert {39, 79, 80, 89, 90, 179, 180} == edges and {max(lengths) for lengths in u.TAIL_LENGTHS} == {54, 55, 126, 127}
    r = lambda S, **kw: u.route(S, 9, **kw)
    assert r(179) == dict(rows=True, ppw=1, tail=False, raised=True) and not r(180)["rows"]
    assert r(89, shared=True)["ppw"] == 2 and r(90, shared=True)["ppw"] == 1
    assert not r(39, shared=True)["raised"] and r(79, shared=True)["raised"] and not r(79)["raised"] and r(80)["raised"]
    assert r(54, sampling=True) == dict(rows=True, ppw=1, tail=True, raised=False) and r(55, sampling=True)["raised"]
    assert r(126, sampling=True)["tail"] and r(127, sampling=True) == dict(rows=True, ppw=1, tail=False, raised=True)
    # the staging loops' second and third trip: lanes beyond 64 and beyond 128 segments
    assert any(64 < S <= 128 for lengths in u.SIZE_EDGE_LENGTHS for S in lengths) and any(S > 128 for S in u.LONGEST_ROWS)

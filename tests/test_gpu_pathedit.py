"""mrs_tg_plan_preprocess_path / mrs_tg_plan_insert_midpoints / mrs_tg_plan_path_edit_vjp on the GPU (thin_path_kernel,
insert_midpoints_kernel, vertex_offsets_kernel, edit_write_kernel, path_edit_vjp_kernel) and
autograd.preprocess_path / insert_midpoints on top of them.  The expected values are the CPU harness's
(tests/host/pathedit_harness.cpp runs the same header) and the oracle's, computed inside the tests; every comparison is bit for
bit: both sides run the same operations without contraction.  NaN is ordinary data here: nothing provokes a fault."""
import itertools

import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd
from tests import deviation_util as du
from tests import pathedit_util as pu

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL, BSENTINEL = -777.25, -7, 201
GUARD = 5          # rows behind the upper bound of an output, which nothing may write either
MAX_DEVIATION = 0.05


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)).cuda()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return pu.build_harness(tmp_path_factory.mktemp("pathedit_gpu"))


def _pack(paths, stops):
    so = np.concatenate([[0], np.cumsum([w.shape[0] - 1 for w in paths])]).astype(np.int32)
    return so, np.concatenate(paths), np.concatenate(stops).astype(np.uint8)


class _Outputs:
    """the outputs of one edit call, prefilled with sentinels, GUARD rows longer than the call's upper bound; `want` says which
    optional ones are passed at all"""

    def __init__(self, n_paths, upper, want=("stop", "source", "inserted")):
        self.upper = upper
        self.offsets = torch.full((n_paths + 1 + GUARD,), ISENTINEL, dtype=torch.int32, device="cuda")
        self.rows = torch.full((upper + GUARD, 4), SENTINEL, dtype=torch.float64, device="cuda")
        self.stop = torch.full((upper + GUARD,), BSENTINEL, dtype=torch.uint8, device="cuda") if "stop" in want else None
        self.source = torch.full((upper + GUARD,), ISENTINEL, dtype=torch.int32, device="cuda") if "source" in want else None
        self.inserted = torch.full((upper + GUARD,), BSENTINEL, dtype=torch.uint8, device="cuda") if "inserted" in want else None

    def read(self, n_paths):
        """-> dict of numpy arrays cut at the total; asserts that nothing at or behind the total was written"""
        torch.cuda.synchronize()
        off = self.offsets.cpu().numpy()
        assert np.all(off[n_paths + 1:] == ISENTINEL)
        off = off[:n_paths + 1].copy()
        total = int(off[-1])
        assert off[0] == 0 and 0 <= total <= self.upper
        out = dict(offsets=off, total=total)
        for name, t, fill in (("rows", self.rows, SENTINEL), ("stop", self.stop, BSENTINEL), ("source", self.source, ISENTINEL),
                              ("inserted", self.inserted, BSENTINEL)):
            if t is None:
                continue
            host = t.cpu().numpy()
            assert np.all(host[total:] == fill), "%s: written at or behind the final offset" % name
            out[name] = host[:total].copy()
        return out


def _thin(ctx, problems, want=("stop", "source")):
    """one mrs_tg_plan_preprocess_path on the problems as a batch (one min_distance and straightener for all)"""
    so, wp, stop = _pack([p["waypoints"] for p in problems], [p["stop_at"] for p in problems])
    p0 = problems[0]
    on = p0["straightener"] is not None
    dev, hdg = p0["straightener"] if on else (0.0, 0.0)
    plan = api.Plan(ctx, so)
    try:
        out = _Outputs(plan.n_paths, wp.shape[0], want)
        plan.preprocess_path(_dev(wp), out.offsets, out.rows, min_waypoint_distance=p0["min_distance"], stop_at=_dev(stop),
                             straightener_enabled=on, straightener_max_deviation=dev, straightener_max_hdg_deviation=hdg,
                             stop_at_out=out.stop, source=out.source)
        return out.read(plan.n_paths), so
    finally:
        plan.close()


def _subdivide(ctx, problems, active=None, want=("stop", "source", "inserted"), max_deviation=MAX_DEVIATION, segment_max=None):
    """one mrs_tg_plan_insert_midpoints on the problems as a batch; segment_max from the flags unless given: above the bound
    where unsafe; exactly the bound, below it or NaN where safe"""
    so, wp, stop = _pack([p["waypoints"] for p in problems], [p["stop_at"] for p in problems])
    if segment_max is None:
        flags = np.concatenate([p["unsafe"] for p in problems])
        safe_values = np.array([max_deviation, 0.5 * max_deviation, np.nan, 0.0])[np.arange(flags.size) % 4]
        segment_max = np.where(flags != 0, max_deviation * (1.0 + 2.0 ** -50), safe_values)
    plan = api.Plan(ctx, so)
    try:
        out = _Outputs(plan.n_paths, wp.shape[0] + int(so[-1]), want)
        plan.insert_midpoints(_dev(wp), _dev(segment_max), max_deviation, out.offsets, out.rows,
                              first_segment=bool(problems[0]["first_segment"]), stop_at=_dev(stop),
                              active=None if active is None else _dev(active, np.uint8), stop_at_out=out.stop, source=out.source,
                              inserted=out.inserted)
        return out.read(plan.n_paths), so
    finally:
        plan.close()


def _expect_packed(got, so, per_path):
    """per_path: dicts(rows, stop_at, source (own numbering), inserted or None) in the batch's order"""
    counts = [e["rows"].shape[0] for e in per_path]
    assert np.array_equal(got["offsets"], np.concatenate([[0], np.cumsum(counts)])), (got["offsets"], counts)
    assert pu.same_bits(got["rows"], np.concatenate([e["rows"] for e in per_path]))
    if "stop" in got:
        assert np.array_equal(got["stop"], np.concatenate([e["stop_at"] for e in per_path]))
    if "source" in got:
        v0 = so[:-1].astype(np.int64) + np.arange(len(per_path))
        assert np.array_equal(got["source"], np.concatenate([e["source"] + v for e, v in zip(per_path, v0)]))
    if "inserted" in got:
        assert np.array_equal(got["inserted"], np.concatenate([e["inserted"] for e in per_path]))


# ---- capability and arguments ---------------------------------------------------------------------------------------------

def test_capability_symbols_and_kernel_ids(gpu_ctx):
    assert api.CAP_PATH_EDIT == 4096 and api.capabilities() & api.CAP_PATH_EDIT
    assert (api.KERNEL_PREPROCESS_PATH, api.KERNEL_INSERT_MIDPOINTS, api.KERNEL_PATH_EDIT_VJP) == (20, 21, 22)
    lib = api.load_library()
    for name in ("mrs_tg_plan_preprocess_path", "mrs_tg_plan_insert_midpoints", "mrs_tg_plan_path_edit_vjp"):
        assert hasattr(lib, name) and name in api.EXPORTED_SYMBOLS
    assert lib.mrs_tg_abi_version() == 5
    rng = np.random.default_rng(3)
    problems = [pu.subdivide_problem(pu.random_path(rng, 11), rng.integers(0, 2, 10), 1) for _ in range(70)]
    try:
        gpu_ctx.set_profiling(True)
        api.kernel_trace_reset()
        got, so = _subdivide(gpu_ctx, problems)
        _thin(gpu_ctx, [pu.thin_problem(p["waypoints"], 5.0) for p in problems])
        mine = ("insert_midpoints_kernel", "vertex_offsets_kernel", "edit_write_kernel<true>", "thin_path_kernel",
                "vertex_offsets_kernel", "edit_write_kernel<false>")
        assert tuple(k for k in api.kernel_trace() if k in mine) == mine, api.kernel_trace()
        for kernel in (api.KERNEL_PREPROCESS_PATH, api.KERNEL_INSERT_MIDPOINTS):
            assert gpu_ctx.last_kernel_ms(kernel) > 0, kernel
    finally:
        gpu_ctx.set_profiling(False)


def test_argument_errors_come_before_any_launch(gpu_ctx):
    rng = np.random.default_rng(4)
    w = pu.random_path(rng, 6)
    plan = api.Plan(gpu_ctx, np.array([0, 5], dtype=np.int32))
    try:
        wp, seg_max = _dev(w), _dev(np.full(5, 1.0))
        out = _Outputs(1, 11)
        nan = float("nan")

        def thin(**kw):
            a = dict(waypoints=wp, vertex_offsets=out.offsets, waypoints_out=out.rows, min_waypoint_distance=0.05,
                     straightener_enabled=True, straightener_max_deviation=0.1, straightener_max_hdg_deviation=0.1,
                     stop_at_out=out.stop, source=out.source)
            a.update(kw)
            with pytest.raises(api.MrsTgError):
                plan.preprocess_path(**a)

        def subdivide(**kw):
            a = dict(waypoints=wp, segment_max=seg_max, max_deviation=0.05, vertex_offsets=out.offsets, waypoints_out=out.rows,
                     stop_at_out=out.stop, source=out.source, inserted=out.inserted)
            a.update(kw)
            with pytest.raises(api.MrsTgError):
                plan.insert_midpoints(**a)

        for kw in (dict(waypoints=None), dict(vertex_offsets=None), dict(waypoints_out=None), dict(min_waypoint_distance=-1e-300),
                   dict(min_waypoint_distance=nan), dict(straightener_max_deviation=-1.0), dict(straightener_max_deviation=nan),
                   dict(straightener_max_hdg_deviation=-0.1), dict(straightener_max_hdg_deviation=nan)):
            thin(**kw)
        for kw in (dict(waypoints=None), dict(segment_max=None), dict(vertex_offsets=None), dict(waypoints_out=None),
                   dict(max_deviation=-0.05), dict(max_deviation=nan)):
            subdivide(**kw)
        g = torch.zeros((6, 4), dtype=torch.float64, device="cuda")
        for kw in (dict(vertex_offsets=None), dict(source=None), dict(grad_waypoints_edited=None), dict(grad_waypoints=None)):
            a = dict(vertex_offsets=out.offsets, source=out.source, grad_waypoints_edited=out.rows, grad_waypoints=g)
            a.update(kw)
            with pytest.raises(api.MrsTgError):
                plan.path_edit_vjp(**a)
        torch.cuda.synchronize()
        for t, fill in ((out.offsets, ISENTINEL), (out.rows, SENTINEL), (out.stop, BSENTINEL), (out.source, ISENTINEL),
                        (out.inserted, BSENTINEL)):
            assert bool(torch.all(t == fill))        # nothing ran
        assert bool(torch.all(g == 0.0))
    finally:
        plan.close()


# ---- thinning -------------------------------------------------------------------------------------------------------------

def _thin_batch(straightener):
    """the ragged batch of the issue: V in {2, 3, 64, 65, 66, 129, 130, 257}, the fixed cases and the window placements among
    them, one min_waypoint_distance (5.0) for all"""
    rng = np.random.default_rng(21)
    problems = [dict(p, min_distance=5.0, straightener=straightener) for p, _ in pu.fixed_thin_cases()]
    for V, kept in pu.window_cases(rng):
        w, _ = pu.path_from_kept(V, kept, rng)
        problems.append(pu.thin_problem(w, 5.0, stop_at=rng.integers(0, 2, V), straightener=straightener, name="window_%d" % V))
    for V in (3, 64, 66, 129, 257):     # clusters between long steps, nearly straight: the straightener's tests all decide
        w = pu.random_clustered_path(rng, V, straight=True)
        w[:, :3] *= 10.0
        problems.append(pu.thin_problem(w, 5.0, stop_at=rng.integers(0, 2, V), straightener=straightener, name="clustered_%d" % V))
    assert {p["waypoints"].shape[0] for p in problems} == {2, 3, 64, 65, 66, 129, 130, 257}
    return problems


@pytest.mark.parametrize("straightener", [None, (0.2, 0.3)], ids=["distance_only", "straightener"])
def test_thinning_of_a_ragged_batch_in_bits(gpu_ctx, harness, straightener):
    problems = _thin_batch(straightener)
    cpu = pu.run_thin(harness, problems)
    expected = []
    for p, c in zip(problems, cpu):
        rows, stop = pu.oracle_thin(p)
        assert np.array_equal(c["serial"], c["window"]) and pu.same_bits(p["waypoints"][c["window"]], rows), p["name"]
        expected.append(dict(rows=rows, stop_at=stop, source=c["window"], inserted=None))
    got, so = _thin(gpu_ctx, problems)
    _expect_packed(got, so, expected)
    dropped = sum(p["waypoints"].shape[0] - e["rows"].shape[0] for p, e in zip(problems, expected))
    assert dropped > 1000 and any(e["rows"].shape[0] == p["waypoints"].shape[0] for p, e in zip(problems, expected))
    if straightener is None:
        for (V, kept), p, e in zip(pu.window_cases(None), problems[len(pu.fixed_thin_cases()):], expected[len(pu.fixed_thin_cases()):]):
            assert np.array_equal(e["source"], sorted(set(kept) | {0, V - 1})), p["name"]


# ---- subdivision ----------------------------------------------------------------------------------------------------------

def _subdivide_batch(first_segment):
    rng = np.random.default_rng(31)
    problems = []
    for S in (1, 2, 63, 64, 65, 128, 256):
        w = pu.random_path(rng, S + 1)
        stop = rng.integers(0, 2, S + 1)
        for pattern, flags in pu.flag_patterns(S, rng).items():
            problems.append(pu.subdivide_problem(w, flags, first_segment, stop_at=stop, name="S%d_%s" % (S, pattern)))
    seam = pu.seam_path()
    problems.append(pu.subdivide_problem(seam, np.ones(seam.shape[0] - 1), first_segment, name="seam"))
    return problems


@pytest.mark.parametrize("first_segment", [0, 1])
def test_subdivision_at_the_chunk_edges_in_bits(gpu_ctx, harness, first_segment):
    problems = _subdivide_batch(first_segment)
    active = (np.arange(len(problems)) % 3 != 2).astype(np.uint8)
    as_run = [p if a else dict(p, unsafe=np.zeros_like(p["unsafe"])) for p, a in zip(problems, active)]   # inactive: a copy
    expected = pu.run_subdivide(harness, as_run)
    for p, e in zip(as_run, expected):
        rows, stop = pu.reference_subdivide(p)
        assert pu.same_bits(e["rows"], rows) and np.array_equal(e["stop_at"], stop), p["name"]
    got, so = _subdivide(gpu_ctx, problems, active=active)
    _expect_packed(got, so, expected)
    sizes = {p["name"]: e["rows"].shape[0] for p, e in zip(problems, expected)}
    assert max(sizes.values()) == 512 + first_segment and got["inserted"].sum() > 500
    # every path active, no active array
    expected = pu.run_subdivide(harness, problems)
    got, so = _subdivide(gpu_ctx, problems, active=None)
    _expect_packed(got, so, expected)
    assert {e["rows"].shape[0] for p, e in zip(problems, expected) if p["name"] == "S256_all"} == {512 + first_segment}


def _scan_problems(n_paths, seed):
    """ragged paths of 50 / 51 segments with random flags: the counts differ from path to path"""
    rng = np.random.default_rng(seed)
    problems = []
    for k in range(n_paths):
        S = 50 + (k % 2 if n_paths > 2 else 0)
        problems.append(pu.subdivide_problem(pu.random_path(rng, S + 1), rng.integers(0, 2, S), 1, stop_at=rng.integers(0, 2, S + 1)))
    return problems


@pytest.mark.parametrize("n_paths", [1, 2, pu.SCAN_CHUNK - 1, pu.SCAN_CHUNK, pu.SCAN_CHUNK + 1])
def test_offsets_across_the_scan_chunk(gpu_ctx, n_paths):
    problems = _scan_problems(n_paths, 40 + n_paths)
    got, so = _subdivide(gpu_ctx, problems)
    counts = np.array([p["waypoints"].shape[0] + int(p["unsafe"].sum()) for p in problems])   # (first_segment = 1: the flags decide)
    assert np.array_equal(got["offsets"], np.concatenate([[0], np.cumsum(counts)]))
    if n_paths >= pu.SCAN_CHUNK - 1:
        assert got["total"] > 2 ** 16
    wp = np.concatenate([p["waypoints"] for p in problems])
    copies = got["inserted"] == 0
    assert pu.same_bits(got["rows"][copies], wp) and np.array_equal(got["source"][copies], np.arange(wp.shape[0]))
    assert np.array_equal(got["source"][~copies], got["source"][np.flatnonzero(~copies) - 1])
    assert np.array_equal(got["stop"][copies], np.concatenate([p["stop_at"] for p in problems])) and not got["stop"][~copies].any()
    # the thinning's counts through the same scan: every path keeps its two ends and every fifth vertex in between
    rng = np.random.default_rng(n_paths)
    thin = []
    for p in problems:
        V = p["waypoints"].shape[0]
        w, kept = pu.path_from_kept(V, list(range(0, V, 5)), rng)
        thin.append((pu.thin_problem(w, 5.0), kept))
    got, so = _thin(gpu_ctx, [t for t, _ in thin])
    assert np.array_equal(got["offsets"], np.concatenate([[0], np.cumsum([k.size for _, k in thin])]))
    v0 = so[:-1].astype(np.int64) + np.arange(n_paths)
    assert np.array_equal(got["source"], np.concatenate([k + v for (_, k), v in zip(thin, v0)]))


def test_optional_outputs_in_any_combination(gpu_ctx, harness):
    rng = np.random.default_rng(50)
    problems = [pu.subdivide_problem(pu.random_path(rng, V), rng.integers(0, 2, V - 1), 0, stop_at=rng.integers(0, 2, V))
                for V in (2, 3, 9, 66, 130)]
    expected = pu.run_subdivide(harness, problems)
    thin = [pu.thin_problem(*pu.path_from_kept(p["waypoints"].shape[0], [0, 1], rng)[:1], 5.0, stop_at=p["stop_at"]) for p in problems]
    thin_expected = [dict(rows=p["waypoints"][c["window"]], stop_at=p["stop_at"][c["window"]], source=c["window"], inserted=None)
                     for p, c in zip(thin, pu.run_thin(harness, thin))]
    names = ("stop", "source", "inserted")
    for r in range(len(names) + 1):
        for want in itertools.combinations(names, r):
            got, so = _subdivide(gpu_ctx, problems, want=want)
            assert set(got) == {"offsets", "total", "rows"} | set(want)
            _expect_packed(got, so, expected)
            if "inserted" not in want:
                got, so = _thin(gpu_ctx, thin, want=want)
                _expect_packed(got, so, thin_expected)


# ---- backward pass --------------------------------------------------------------------------------------------------------

def _vjp(ctx, so, got, upstream, with_inserted):
    plan = api.Plan(ctx, so)
    try:
        n_v = int(so[-1]) + plan.n_paths
        full = torch.full((n_v + 2, 4), SENTINEL, dtype=torch.float64, device="cuda")
        plan.path_edit_vjp(_dev(got["offsets"]), _dev(got["source"]), _dev(upstream), full[1:n_v + 1],
                           inserted=_dev(got["inserted"]) if with_inserted else None)
        torch.cuda.synchronize()
        host = full.cpu().numpy()
        assert np.all(host[0] == SENTINEL) and np.all(host[-1] == SENTINEL)
        return host[1:-1].copy()
    finally:
        plan.close()


def _reference_vjp_batch(so, got, upstream, with_inserted):
    out = []
    for p in range(so.size - 1):
        r0, r1 = int(got["offsets"][p]), int(got["offsets"][p + 1])
        v0, n_in = int(so[p]) + p, int(so[p + 1] - so[p]) + 1
        out.append(pu.reference_vjp(n_in, got["source"][r0:r1] - v0, got["inserted"][r0:r1] if with_inserted else None,
                                    upstream[r0:r1]))
    return np.concatenate(out)


def test_backward_pass_of_the_subdivision_in_bits(gpu_ctx):
    problems = _subdivide_batch(1)
    active = (np.arange(len(problems)) % 4 != 2).astype(np.uint8)
    got, so = _subdivide(gpu_ctx, problems, active=active)
    rng = np.random.default_rng(60)
    up = pu.dyadic(rng, 4 * got["total"]).reshape(-1, 4) * (1.0 + 2.0 ** -40)     # (the halves and the sums round)
    g = _vjp(gpu_ctx, so, got, up, True)
    assert pu.same_bits(g, _reference_vjp_batch(so, got, up, True))
    assert abs(g.sum() - up.sum()) < 1e-9 * np.abs(up).sum()      # the weights of every edited row sum to one


def test_backward_pass_of_the_thinning_in_bits(gpu_ctx):
    problems = _thin_batch(None)
    got, so = _thin(gpu_ctx, problems)
    rng = np.random.default_rng(61)
    up = pu.dyadic(rng, 4 * got["total"]).reshape(-1, 4)
    g = _vjp(gpu_ctx, so, got, up, False)
    assert pu.same_bits(g, _reference_vjp_batch(so, got, up, False))
    dropped = np.setdiff1d(np.arange(g.shape[0]), got["source"])
    assert dropped.size > 1000 and np.all(pu.bits(g[dropped]) == 0)       # a dropped vertex gets a zero row, +0.0
    assert pu.same_bits(g[got["source"]], up)                             # a kept one its copy's row


@pytest.mark.parametrize("step", ["thin", "subdivide"])
def test_gradient_against_central_differences(gpu_ctx, step):
    """one 6-vertex path; the map is linear in x, y, z, so the differences are exact up to the rounding of the step: 1e-9"""
    rng = np.random.default_rng(70)
    plan = api.Plan(gpu_ctx, np.array([0, 5], dtype=np.int32))
    try:
        if step == "thin":
            w0, _ = pu.path_from_kept(6, [0, 2, 3, 5], rng, spacing=1.0)
            run = lambda w: autograd.preprocess_path(plan, w, min_waypoint_distance=0.5)[1]
        else:
            w0 = pu.random_path(rng, 6)
            seg_max = _dev(np.array([0.2, 0.0, 0.2, 0.2, 0.01]))
            run = lambda w: autograd.insert_midpoints(plan, w, seg_max, MAX_DEVIATION, first_segment=True)[1]
        w = _dev(w0).requires_grad_()
        edited = run(w)
        assert edited.shape[0] == (4 if step == "thin" else 9)
        c = _dev(rng.uniform(-1, 1, size=tuple(edited.shape)))
        (edited * c).sum().backward()
        grad = w.grad.cpu().numpy()
        h = 2.0 ** -10
        for v in range(6):
            for k in range(3):
                d = np.zeros_like(w0)
                d[v, k] = h
                hi = float((run(_dev(w0 + d)).detach() * c).sum())
                lo = float((run(_dev(w0 - d)).detach() * c).sum())
                assert abs((hi - lo) / (2 * h) - grad[v, k]) < 1e-9, (v, k, (hi - lo) / (2 * h), grad[v, k])
        if step == "thin":
            assert np.all(grad[[1, 4]] == 0.0)
    finally:
        plan.close()


# ---- the chain deviation -> subdivision -------------------------------------------------------------------------------------

@pytest.mark.parametrize("first_segment", [0, 1])
def test_deviation_then_subdivision_is_the_policy_layer(gpu_ctx, harness, first_segment):
    cap = 128
    problems = []
    for k, S in enumerate([1, 1, 2, 3, 4, 7, 12, 5, 9, 2]):
        w = np.zeros((S + 1, 4))
        w[:, :3] = du.polyline(S, 300 + k)
        w[:, 3] = np.random.default_rng(k).uniform(-7, 7, S + 1)
        n = 20 + 7 * S
        s = np.zeros((n, 4))
        s[:, :3] = du.walk(w, n, [0.0, 0.03, 0.08, 0.2][k % 4], 400 + k)
        problems.append(dict(waypoints=w, stop_at=np.random.default_rng(50 + k).integers(0, 2, S + 1).astype(np.uint8), samples=s,
                             first_segment=first_segment, max_deviation=MAX_DEVIATION))
    expected = pu.run_chain(harness, problems)
    so, wp, stop = _pack([p["waypoints"] for p in problems], [p["stop_at"] for p in problems])
    P = len(problems)
    samples = np.zeros((P, cap, 4))
    for p, prob in enumerate(problems):
        samples[p, :prob["samples"].shape[0]] = prob["samples"]
    n_samples = np.array([prob["samples"].shape[0] for prob in problems], dtype=np.int32)
    plan = api.Plan(gpu_ctx, so)
    try:
        seg_max = torch.full((int(so[-1]),), SENTINEL, dtype=torch.float64, device="cuda")
        plan.path_deviation(_dev(samples), _dev(n_samples), _dev(wp), first_segment=bool(first_segment), segment_max=seg_max)
        out = _Outputs(P, wp.shape[0] + int(so[-1]))
        plan.insert_midpoints(_dev(wp), seg_max, MAX_DEVIATION, out.offsets, out.rows, first_segment=bool(first_segment),
                              stop_at=_dev(stop), stop_at_out=out.stop, source=out.source, inserted=out.inserted)
        got = out.read(P)
    finally:
        plan.close()
    assert np.array_equal(got["offsets"], np.concatenate([[0], np.cumsum([e["rows"].shape[0] for e in expected])]))
    assert pu.same_bits(got["rows"], np.concatenate([e["rows"] for e in expected]))
    assert np.array_equal(got["stop"], np.concatenate([e["stop_at"] for e in expected]))
    assert any(e["is_safe"] for e in expected) and got["inserted"].sum() >= 5

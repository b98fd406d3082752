"""sample_path_walk (csrc/mrs_tg_sampling.hpp) on the GPU at the edges the solved trajectories of the other sampler tests never
reach: samples exactly on a segment boundary, remainders carried through several segments, zero-length and exhausted segments,
an end on a multiple of dt, chunks of 61 .. 66 samples, 192 / 193 parked samples, capacities at N - 1, N, N + 1 and on chunk and
buffer edges, the last entries of the accumulated-time table, a NaN and an infinite segment time (the ABI takes both: no
sample, and capacity + 1).  The cases and their reference are tests/sampler_walk_util.py (test_sampler_walk_cases.py shows
without a GPU that the replay counts as the oracle does and that each case reaches its edge).

All cases travel as ONE ragged batch (long, short, long; 256 segments put the staging above 64 KB of LDS), sampled at each
case's dt and each of its capacities.  At every call EVERY path is compared with the replay at that dt, whichever case the dt
belongs to: (segment, time) of the backward pass's walk bit for bit, the counts, untouched rows beyond the count, sample_kernel<0>
= order 0 of sample_kernel<4>, and the states equal to the same path's states at the largest capacity.  The values of the cases
whose dt it is are held to horner_bound around exact_state: every sample at capacities 192 and the largest (of a path with
more than 450: the first and last 70 and every 7th between them, which keeps the exactly evaluated rows below 8000), the last 70
below the cut elsewhere; a row whose bits were already checked is not evaluated again.  Every order-0 heading of every path lies
in (-pi, pi] up to the wrap's own rounding (heading_limits).
The table-edge cases' dt (13/32) is sampled at capacities up to 1024 only: a larger capacity would grow that table beyond its
smallest size, which is what they are about."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, problem as pr
from tests import sampler_walk_util as w

pytestmark = pytest.mark.gpu

NAN = float("nan")
TOP = w.STANDARD_CAPACITIES[-1]
LONG, WINDOW, STRIDE = 450, 70, 7   # (7 shares no factor with the 64 lanes of a chunk or the 192 parked samples)
INSIDE = 1.0 - 2.0 ** -50   # state_errors' ratios are right to 2^-52: at or below this a value is inside the bound
DTS = sorted({c[2] for c in w.CASES})


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class _Walk:
    def __init__(self, ctx):
        self.ctx = ctx
        self.coeffs_h = [w.case_coeffs(i) for i in range(len(w.CASES))]
        self.times_h = [np.array(c[1], dtype=np.float64) for c in w.CASES]
        so = np.zeros(len(w.CASES) + 1, dtype=np.int32)
        so[1:] = np.cumsum([t.size for t in self.times_h])
        self.plan = api.Plan(ctx, so)
        self.coeffs = _dev(np.concatenate(self.coeffs_h))
        self.times = _dev(np.concatenate(self.times_h))
        self.P = len(w.CASES)
        self._ref = {}
        self._split = {}
        self.checked = {}       # (dt, path, sample) -> the bits of a states row that passed the exact check
        self.worst = np.zeros(w.N_ORDERS)
        self.n_exact = 0

    def ref(self, p, dt):
        """the replay of path p at dt, up to TOP + 1 samples: (segment [n], time [n], count)"""
        if (p, dt) not in self._ref:
            samples, n = w.replay(w.CASES[p][1], dt, TOP)
            self._ref[p, dt] = (np.array([s for s, _ in samples], dtype=np.int32), np.array([t for _, t in samples], dtype=np.float64), n)
        return self._ref[p, dt]

    def vjp(self, dt, cap):
        seg = torch.full((self.P, cap), -1, dtype=torch.int32, device="cuda")
        tau = torch.full((self.P, cap), NAN, dtype=torch.float64, device="cuda")
        n = torch.full((self.P,), -1, dtype=torch.int32, device="cuda")
        self.plan.sample_states_vjp(self.coeffs, self.times, dt, cap, None, sample_segment=seg, sample_time=tau, n_samples=n)
        torch.cuda.synchronize()
        return seg.cpu().numpy(), tau.cpu().numpy(), n.cpu().numpy()

    def forward(self, dt, cap):
        n_a = torch.full((self.P,), -1, dtype=torch.int32, device="cuda")
        n_b = torch.full((self.P,), -1, dtype=torch.int32, device="cuda")
        states = torch.full((self.P, cap, api.STATE_ORDERS, 4), NAN, dtype=torch.float64, device="cuda")
        samples = torch.full((self.P, cap, 4), NAN, dtype=torch.float64, device="cuda")
        self.plan.sample_states(self.coeffs, self.times, dt, cap, n_a, states)
        self.plan.sample(self.coeffs, self.times, dt, cap, n_b, samples)
        torch.cuda.synchronize()
        return states.cpu().numpy(), n_a.cpu().numpy(), samples.cpu().numpy(), n_b.cpu().numpy()

    def exact_check(self, dt, p, k, row, where):
        key = (dt, p, k)
        bits = row.tobytes()
        if self.checked.get(key) == bits:
            return
        seg, tau, _ = self.ref(p, dt)
        s = int(seg[k])
        if (p, s) not in self._split:
            self._split[p, s] = w.split_segment(self.coeffs_h[p][s])
        r = w.state_errors(self._split[p, s], float(tau[k]), row)
        self.n_exact += 1
        assert np.max(r) <= INSIDE, (where, "sample %d in segment %d at %r" % (k, s, float(tau[k])), "error / bound per order and dimension", r.tolist())
        self.worst = np.maximum(self.worst, np.max(r, axis=1))
        self.checked[key] = bits


@pytest.fixture(scope="module")
def walk(gpu_ctx):
    wk = _Walk(gpu_ctx)
    yield wk
    wk.plan.close()


def _compare_walk(wk, dt, cap, seg, tau, n):
    for p in range(wk.P):
        rs, rt, rn = wk.ref(p, dt)
        where = "case %s (path %d) at dt %r, capacity %d" % (w.CASES[p][0], p, dt, cap)
        assert n[p] == min(rn, cap + 1), (where, "count: expected %d, got %d" % (min(rn, cap + 1), n[p]))
        r = min(rn, cap)
        same = (seg[p, :r] == rs[:r]) & (_bits(tau[p, :r]) == _bits(rt[:r]))
        if not np.all(same):
            k = int(np.argmin(same))
            pytest.fail("%s: sample %d of %d: expected segment %d time %r (%#018x), got segment %d time %r (%#018x); %d samples differ"
                        % (where, k, r, rs[k], float(rt[k]), int(_bits(rt[k:k + 1])[0]), seg[p, k], float(tau[p, k]),
                           int(_bits(tau[p, k:k + 1])[0]), int(np.sum(~same))))
        assert np.all(seg[p, r:] == -1) and np.all(np.isnan(tau[p, r:])), (where, "entries beyond the count were written")


@pytest.mark.parametrize("dt", DTS)
def test_the_walk_and_the_states_at_every_capacity(walk, dt):
    wk = walk
    own = [p for p in range(wk.P) if w.CASES[p][2] == dt]
    caps = w.dt_capacities(dt)
    top = caps[-1]
    assert top == (w.TABLE_CAPACITY if dt == w.TABLE_DT else TOP)
    top_states = None
    for cap in [top] + caps[:-1]:
        seg, tau, n = wk.vjp(dt, cap)
        _compare_walk(wk, dt, cap, seg, tau, n)
        states, n_a, samples, n_b = wk.forward(dt, cap)
        if cap == top:
            top_states = states
            for p in range(wk.P):   # (every other capacity's rows are held to these bits below)
                rs, rt, rn = wk.ref(p, dt)
                r = min(rn, cap)
                over = np.abs(states[p, :r, 0, 3]) > w.heading_limits(wk.coeffs_h[p], rs[:r], rt[:r])
                assert not np.any(over), ("case %s (path %d) at dt %r" % (w.CASES[p][0], p, dt), "order-0 heading outside (-pi, pi] at samples",
                                          np.flatnonzero(over)[:8].tolist(), states[p, :r, 0, 3][over][:8].tolist())
        for p in range(wk.P):
            rs, rt, rn = wk.ref(p, dt)
            where = "case %s (path %d) at dt %r, capacity %d" % (w.CASES[p][0], p, dt, cap)
            assert n_a[p] == n_b[p] == min(rn, cap + 1), (where, "counts of sample_states / sample", n_a[p], n_b[p], min(rn, cap + 1))
            r = min(rn, cap)
            assert np.all(np.isnan(states[p, r:])) and np.all(np.isnan(samples[p, r:])), (where, "rows at or beyond min(n, capacity) were written")
            assert np.array_equal(_bits(samples[p, :r]), _bits(states[p, :r, 0])), (where, "sample_kernel<0> is not order 0 of the states")
            # the same (segment, time) at the same coefficients: the bits of the largest capacity's rows
            assert np.array_equal(_bits(states[p, :r]), _bits(top_states[p, :r])), (where, "states differ from those at capacity %d" % top)
            if p not in own:
                continue
            if cap in (192, top):
                rows = range(r) if r <= LONG else list(range(WINDOW)) + list(range(WINDOW, r - WINDOW, STRIDE)) + list(range(r - WINDOW, r))
            else:
                rows = range(max(0, r - WINDOW), r)
            for k in rows:
                wk.exact_check(dt, p, k, states[p, k], where)
    print("WALK EDGES dt %r: %d cases, capacities %s; %d rows evaluated exactly so far; worst error / bound per order so far %s"
          % (dt, len(own), caps, wk.n_exact, ["%.3f" % x for x in wk.worst]))


@pytest.mark.parametrize("dt", DTS)
def test_the_counts_only_calls(walk, dt):
    """capacity 0: "more than fit" = 1 for every path with a sample, 0 for the others, from all three kernels"""
    wk = walk
    want = np.array([min(wk.ref(p, dt)[2], 1) for p in range(wk.P)], dtype=np.int32)
    assert want[[c[0] for c in w.CASES].index("no_sample")] == 0 and want[[c[0] for c in w.CASES].index("nan_time")] == 0 and want.sum() == wk.P - 2
    for call in ("states", "sample", "vjp"):
        n = torch.full((wk.P,), -1, dtype=torch.int32, device="cuda")
        if call == "states":
            wk.plan.sample_states(wk.coeffs, wk.times, dt, 0, n, None)
        elif call == "sample":
            wk.plan.sample(wk.coeffs, wk.times, dt, 0, n, None)
        else:
            wk.plan.sample_states_vjp(wk.coeffs, wk.times, dt, 0, None, n_samples=n)
        torch.cuda.synchronize()
        assert np.array_equal(n.cpu().numpy(), want), (call, dt, n.cpu().numpy())


def test_these_calls_run_the_samplers_own_kernels(walk):
    wk = walk
    api.kernel_trace_reset()
    wk.forward(0.2, 64)
    trace = api.kernel_trace()
    assert sum(k.startswith("sample_kernel<") for k in trace) == 2 and not any("vjp" in k or k.startswith("solve") for k in trace), trace
    api.kernel_trace_reset()
    wk.vjp(0.2, 64)
    trace = api.kernel_trace()
    assert sum(k.startswith("sample_vjp_kernel<") for k in trace) == 1 and not any(k.startswith("sample_kernel") for k in trace), trace


# ---- the tail of solve_rows_kernel: the walk on times the caller dictates, sub-dt segments among them

TAIL_TIMES = ([1.0, 0.05, 0.06, 0.07, 1.0], [0.1] * 12, [15.25, 15.5, 16.0, 16.25])
TAIL_DTS = (0.2, 0.1, 0.25)


@pytest.mark.parametrize("dt", TAIL_DTS)
@pytest.mark.parametrize("cap", [64, 512])
def test_the_solve_kernels_tail_walks_the_same_way(gpu_ctx, dt, cap):
    """A fixed-times solve with sampling of three short random-walk paths (5, 12 and 4 segments; segments of 0.05 .. 0.07 s and
    0.1 s lie below the sampling periods): the samples come from the tail of solve_rows_kernel, no sampler launch.  The solve
    takes segments of 0.05 s as they are."""
    parts = [pr.build_vertices(pr.random_walk_waypoints(len(t), 4400 + i), pr.SNAP) for i, t in enumerate(TAIL_TIMES)]
    batch = pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (len(parts), 1)))
    seg_times = np.concatenate([np.array(t, dtype=np.float64) for t in TAIL_TIMES])
    assert seg_times.min() < min(TAIL_DTS) and np.all(seg_times > 0)
    api.kernel_trace_reset()
    out = gpu_ctx.solve_batch(batch, seg_times, sampling_dt=dt, sample_capacity=cap)
    trace = api.kernel_trace()
    assert any(k.startswith("solve_rows_kernel") for k in trace) and not any(k.startswith("sample_kernel") for k in trace), trace
    assert np.array_equal(out["times"], seg_times) and np.all(out["status"] > 0) and np.all(np.isfinite(out["coeffs"]))
    so = batch.seg_offsets
    plan = api.Plan(gpu_ctx, so)
    try:
        n_dev = torch.full((batch.n_paths,), -1, dtype=torch.int32, device="cuda")
        samples = torch.full((batch.n_paths, cap, 4), NAN, dtype=torch.float64, device="cuda")
        plan.sample(_dev(out["coeffs"]), _dev(out["times"]), dt, cap, n_dev, samples)
        torch.cuda.synchronize()
    finally:
        plan.close()
    separate, n_separate = samples.cpu().numpy(), n_dev.cpu().numpy()
    worst = 0.0
    for p in range(batch.n_paths):
        where = "path %d at dt %r, capacity %d" % (p, dt, cap)
        ref, rn = w.replay(out["times"][so[p]:so[p + 1]], dt, cap)
        assert out["n_samples"][p] == n_separate[p] == rn, (where, out["n_samples"][p], n_separate[p], rn)
        r = min(rn, cap)
        assert np.array_equal(_bits(out["samples"][p, :r]), _bits(separate[p, :r])), (where, "the tail's samples are not plan.sample's")
        for k in range(r):
            s, tau = ref[k]
            ratios = w.state_errors(out["coeffs"][so[p] + s], tau, out["samples"][p, k])
            assert np.max(ratios) <= INSIDE, (where, "sample %d in segment %d at %r" % (k, s, tau), ratios.tolist())
            worst = max(worst, float(np.max(ratios)))
    print("WALK EDGES solve tail dt %r capacity %d: counts %s, worst error / bound %.3f" % (dt, cap, out["n_samples"].tolist(), worst))

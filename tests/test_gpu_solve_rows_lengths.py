"""solve_rows_kernel (csrc/mrs_tg_rows.hip, one lane per unknown) at the lengths where its schedule changes, every path against
the oracle in 113 bits.

The kernel solves every fixed-times batch below 6144 paths, every ragged batch and every single request.  What runs only at
particular lengths is held here (tests/solve_rows_util.py has the batches and a host statement of the schedule;
test_solve_rows_cases.py shows without a GPU that the batches reach these edges and that the reference side holds):

  * every length 1 .. 40, three paths each (wmax 0 .. 20: every arm of the forward and backward switches with and without a
    refill, the second trip round the quads, sides of unequal length, a short side whose quad 0 starts at the middle vertex),
    for d = 4, 3, 2 as rest-to-rest, moving start and stop_at every third interior vertex, and mixed batches for d = 4 and 2;
  * the size rules of rows_lds_bytes: 39 / 79 | 80 (the 64 KB default limit at one path per wavefront, 39 | 40 at two),
    89 | 90 (two paths per wavefront), 179 | 180 (the kernel applies at all), each longest path with much shorter companions in
    its LDS layout, with 65, 128 / 129 and 179 / 180 segments in the staging loops' second and third trip;
  * the same bits whatever the company: two paths per wavefront (MRS_TG_FLAG_SHARED_DEVICE), a path alone in a one-path plan
    (Smax = S, its own wmax, other LDS offsets), and the grouped dispatch (solve_rows_group_kernel) above 64 KB;
  * the sampling tail at 54 | 55 (64 KB with the sampler's areas) and 126 | 127 (the tail no longer fits: the sampler's own launch).

Gates (those of test_gpu_solve_16_to_24_segments.py; e_h = HIP against 113 bits, e_o = the double-precision oracle against 113
bits, tests/util.py::coeff_error per path; no path is excused: test_solve_rows_cases.py holds e_o <= 1e-4 on every path):

  1. every path: e_h <= 10 * max(e_o, P99(e_o) of its batch); relative cost error against 113 bits <= max(1e-9, 10 * e_o);
  2. median(e_h) <= 10 * median(e_o);
  3. statuses all 1;
  4. continuity and constraint defects < 1e-9 on every path.

Every case prints one ERR line (median / P99 / max of e_h, then of e_o, the worst e_h / max(e_o, P99(e_o)), the worst relative
cost error).  Measured on an MI355X, every case passing (profiles/solve_rows_lengths.txt has the same lines and the CPU side);
the comparisons of bits (two paths per wavefront, alone, grouped, with and without sampling) found no difference anywhere:

  case                          kernel                   e_h median / P99 / max             e_o median / P99 / max             worst ratio  cost
  every-4-rest                  solve_rows_kernel<0>     1.54e-14 / 2.29e-12 / 4.18e-11   5.73e-12 / 2.92e-10 / 2.32e-09   0.018        3.38e-11
  every-4-moving                solve_rows_kernel<0>     1.98e-14 / 8.32e-12 / 4.70e-11   5.66e-12 / 2.54e-10 / 9.06e-10   0.0518       1.72e-11
  every-4-stop                  solve_rows_kernel<0>     2.32e-15 / 5.07e-13 / 4.09e-11   1.08e-11 / 8.43e-11 / 1.58e-09   0.0259       3.61e-11
  every-3-rest                  solve_rows_kernel<0>     8.92e-16 / 3.14e-12 / 2.71e-11   2.55e-11 / 9.67e-10 / 1.43e-09   0.028        1.75e-10
  every-3-moving                solve_rows_kernel<0>     9.15e-16 / 1.54e-11 / 2.18e-07   2.61e-11 / 2.01e-09 / 7.32e-06   0.0297       2.02e-10
  every-3-stop                  solve_rows_kernel<0>     5.31e-16 / 1.68e-13 / 8.47e-13   7.31e-11 / 2.24e-09 / 2.67e-09   0.000317     9.76e-11
  every-2-rest                  solve_rows_kernel<0>     1.44e-15 / 1.31e-13 / 1.93e-13   2.06e-09 / 6.28e-08 / 9.85e-08   3.07e-06     5.32e-10
  every-2-moving                solve_rows_kernel<0>     1.06e-15 / 1.58e-13 / 2.45e-13   1.11e-09 / 1.22e-08 / 1.42e-08   2e-05        2.47e-10
  every-2-stop                  solve_rows_kernel<0>     1.15e-15 / 3.62e-14 / 7.35e-14   2.11e-09 / 5.60e-08 / 6.75e-08   1.31e-06     7.00e-10
  mixed-4                       solve_rows_kernel<0>     1.12e-14 / 4.07e-11 / 1.40e-10   3.96e-11 / 5.45e-09 / 3.06e-08   0.0256       1.69e-11
  mixed-2                       solve_rows_kernel<0>     4.29e-15 / 2.61e-13 / 3.59e-13   3.74e-09 / 7.52e-08 / 1.23e-07   4.77e-06     7.56e-10
  edge-39x17x4-4-rest           solve_rows_kernel<0>     1.60e-14 / 2.00e-12 / 2.17e-12   4.38e-12 / 7.75e-11 / 8.35e-11   0.026        2.73e-11
  edge-39x17x4-2-rest           solve_rows_kernel<0>     4.56e-15 / 1.44e-14 / 1.46e-14   3.01e-09 / 4.96e-08 / 5.26e-08   2.77e-07     4.04e-11
  edge-39x17x4-4-moving         solve_rows_kernel<0>     2.49e-14 / 5.77e-14 / 5.91e-14   3.93e-12 / 2.04e-11 / 2.17e-11   0.0029       2.93e-12
  edge-79x33x5-4-rest           solve_rows_kernel<0>     2.87e-14 / 5.82e-12 / 6.31e-12   4.49e-12 / 5.03e-11 / 5.33e-11   0.118        8.25e-12
  edge-79x33x5-2-rest           solve_rows_kernel<0>     2.32e-15 / 4.95e-14 / 5.32e-14   2.01e-09 / 6.01e-08 / 6.47e-08   8.85e-07     9.37e-11
  edge-79x33x5-4-moving         solve_rows_kernel<0>     3.00e-14 / 1.23e-11 / 1.33e-11   4.77e-12 / 8.28e-11 / 8.46e-11   0.157        2.62e-11
  edge-80x33x5-4-rest           solve_rows_kernel<0>     1.81e-14 / 5.94e-13 / 6.28e-13   6.56e-12 / 1.81e-11 / 1.88e-11   0.0334       2.45e-12
  edge-80x33x5-2-rest           solve_rows_kernel<0>     4.69e-15 / 5.17e-14 / 5.52e-14   4.48e-09 / 4.43e-08 / 4.51e-08   1.22e-06     9.46e-11
  edge-80x33x5-4-moving         solve_rows_kernel<0>     4.43e-14 / 9.76e-12 / 1.06e-11   1.04e-11 / 1.03e-09 / 1.12e-09   0.00948      2.11e-12
  edge-89x64x2-4-rest           solve_rows_kernel<0>     5.59e-14 / 2.33e-13 / 2.35e-13   6.05e-12 / 1.39e-11 / 1.39e-11   0.0169       8.89e-12
  edge-89x64x2-2-rest           solve_rows_kernel<0>     4.97e-15 / 3.19e-13 / 3.23e-13   4.58e-09 / 2.46e-08 / 2.51e-08   1.29e-05     1.06e-10
  edge-89x64x2-4-moving         solve_rows_kernel<0>     2.92e-14 / 5.82e-13 / 6.11e-13   3.29e-12 / 3.71e-11 / 3.96e-11   0.0154       2.41e-12
  edge-90x65x1-4-rest           solve_rows_kernel<0>     3.73e-14 / 5.26e-12 / 5.66e-12   2.03e-12 / 6.78e-11 / 7.12e-11   0.0834       7.23e-12
  edge-90x65x1-2-rest           solve_rows_kernel<0>     9.24e-15 / 3.03e-14 / 3.06e-14   1.80e-09 / 2.22e-08 / 2.27e-08   1.38e-06     1.26e-09
  edge-90x65x1-4-moving         solve_rows_kernel<0>     1.54e-14 / 1.67e-13 / 1.73e-13   3.32e-12 / 1.30e-11 / 1.31e-11   0.0133       1.23e-11
  edge-179x128x65x7-4-rest      solve_rows_kernel<0>     6.36e-14 / 1.50e-12 / 1.61e-12   4.59e-12 / 7.52e-11 / 7.96e-11   0.0203       6.88e-12
  edge-179x128x65x7-2-rest      solve_rows_kernel<0>     2.24e-14 / 3.32e-13 / 3.53e-13   3.59e-09 / 1.25e-08 / 1.26e-08   2.82e-05     2.29e-11
  edge-179x128x65x7-4-moving    solve_rows_kernel<0>     4.03e-14 / 1.50e-12 / 1.50e-12   5.36e-12 / 2.90e-11 / 2.99e-11   0.0517       2.18e-12
  edge-180x129x7-4-rest         solve_tile_kernel<true>  6.94e-14 / 1.25e-12 / 1.33e-12   4.86e-12 / 1.73e-11 / 1.81e-11   0.0734       1.37e-11
  edge-180x129x7-2-rest         solve_tile_kernel<true>  9.54e-15 / 1.39e-14 / 1.40e-14   1.60e-09 / 9.71e-09 / 1.01e-08   1.38e-06     2.18e-15
  edge-180x129x7-4-moving       solve_tile_kernel<true>  8.49e-14 / 3.88e-11 / 4.21e-11   3.43e-12 / 3.87e-10 / 4.16e-10   0.101        8.52e-12
  edge-179x128x65x7-2-moving    solve_rows_kernel<0>     5.42e-15 / 3.52e-13 / 3.85e-13   2.06e-09 / 1.06e-08 / 1.11e-08   3.64e-05     6.55e-11
  tail-54x9                     solve_rows_kernel<1>     2.64e-14 / 5.24e-14 / 5.34e-14   8.31e-12 / 1.97e-11 / 1.99e-11   0.00271      2.13e-12
  tail-55x9                     solve_rows_kernel<1>     1.77e-14 / 1.50e-12 / 1.58e-12   3.57e-12 / 8.11e-11 / 8.49e-11   0.0186       2.73e-12
  tail-126x63x3                 solve_rows_kernel<1>     2.27e-14 / 8.28e-14 / 8.45e-14   5.38e-12 / 2.85e-11 / 3.03e-11   0.00297      2.08e-12
  tail-127x64x3                 solve_rows_kernel<0>     2.16e-14 / 1.81e-13 / 1.84e-13   5.34e-12 / 1.02e-11 / 1.03e-11   0.0181       1.32e-11

The reference's side (CPU, every path; worst e_o): every length d = 4 / 3 / 2: 2.3e-9 / 7.3e-6 (a moving start at 29 segments;
2.7e-9 without it) / 9.9e-8; mixed d = 4 / 2: 3.1e-8 / 1.2e-7; size edges d = 4 / 2: 1.1e-9 / 6.5e-8; sampling-tail batches: 8.5e-11.
"""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api
from tests import solve_rows_util as u
from tests import util

pytestmark = pytest.mark.gpu

DEFECT_BOUND = 1e-9         # gate 4 (the project's bound: tests/test_gpu_round6.py)
BEYOND_DOUBLE = 1e-4
ROWS, ROWS_TAIL, GROUP, SAMPLER = "solve_rows_kernel<0>", "solve_rows_kernel<1>", "solve_rows_group_kernel", "sample_kernel"
NAN = float("nan")


def _solve_kernels(trace):
    return [k for k in trace if k.startswith("solve_")]


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("coeffs", "cost", "status"))


def _traced(ctx, batch, times, **opts):
    api.kernel_trace_reset()
    out = ctx.solve_batch(batch, times, **opts)
    trace = api.kernel_trace()
    assert np.array_equal(out["times"], times)
    return out, trace


def _explain(ctx, batch, group_size=0, **opts):
    """Plan.explain of the solve, and the plan's order"""
    plan = api.Plan(ctx, batch.seg_offsets)
    try:
        names = plan.explain(api.default_options(derivative_to_optimize=batch.derivative_to_optimize, **opts), group_size)
        return names, np.array(plan.order)
    finally:
        plan.close()


def _gates(name, kernel, ref, out):
    batch, so, e_o = ref.batch, ref.batch.seg_offsets, ref.e_o
    e_h = u.path_errors(out["coeffs"], ref.ref_q["coeffs"], so)
    p99 = float(np.percentile(e_o, 99))
    floor = np.maximum(e_o, p99)
    ratio = e_h / floor
    cost_err = np.abs(out["cost"] - ref.ref_q["cost"]) / np.abs(ref.ref_q["cost"])
    print("ERR %-30s %-22s e_h median %.2e P99 %.2e max %.2e | e_o median %.2e P99 %.2e max %.2e | worst e_h / max(e_o, P99) %.3g | cost %.2e"
          % ((name, kernel) + u.stats(e_h) + u.stats(e_o) + (float(ratio.max()), float(cost_err.max()))))
    # 3, and the reference side's conditions
    assert np.all(ref.ref_q["status"] == 1) and np.all(ref.ref_d["status"] == 1) and e_o.max() <= BEYOND_DOUBLE
    assert np.all(out["status"] == 1), np.nonzero(out["status"] != 1)[0][:8]
    assert np.all(np.isfinite(out["coeffs"])) and np.all(np.isfinite(out["cost"]))
    # 1
    worst = int(np.argmax(ratio))
    assert np.all(e_h <= 10.0 * floor), (worst, int(so[worst + 1] - so[worst]), e_h[worst], e_o[worst], p99)
    bad = ~(cost_err <= np.maximum(1e-9, 10.0 * e_o))
    assert not bad.any(), (np.nonzero(bad)[0][:8], cost_err[bad][:8], e_o[bad][:8])
    # 2
    assert np.median(e_h) <= 10.0 * np.median(e_o), (np.median(e_h), np.median(e_o))
    # 4
    cd = util.continuity_defect(batch, out["coeffs"], ref.times)
    kd = util.constraint_defect(batch, out["coeffs"], ref.times)
    assert cd < DEFECT_BOUND and kd < DEFECT_BOUND, (cd, kd)


# ---- 1, 2 and 3a: the route, every path against 113 bits, and the same bits at two paths per wavefront
@pytest.mark.parametrize("key", u.EVERY_KEYS + u.EDGE_KEYS, ids=u.key_id)
def test_lengths_against_113_bits(gpu_ctx, key):
    ref = u.reference(key)
    batch = ref.batch
    Smax = int(np.diff(batch.seg_offsets).max())
    model = u.route(Smax, batch.n_paths)
    assert model["rows"] == (Smax <= 179)
    out, trace = _traced(gpu_ctx, batch, ref.times)
    names, order = _explain(gpu_ctx, batch)
    assert np.array_equal(order, u.plan_order(batch.seg_offsets))    # the host statement of the wavefronts is the plan's
    assert _solve_kernels(names) == _solve_kernels(trace), (names, trace)
    if model["rows"]:
        assert _solve_kernels(trace) == [ROWS], trace
    else:   # 180 segments: the hand-over to the tile / lane kernels, held to the same gates
        assert _solve_kernels(trace) and not any("rows" in k for k in trace), trace
    _gates(u.key_id(key), _solve_kernels(trace)[0], ref, out)
    # two paths per wavefront (from 90 segments the launcher falls back to one)
    shared, trace_s = _traced(gpu_ctx, batch, ref.times, flags=api.FLAG_SHARED_DEVICE)
    assert _solve_kernels(trace_s) == _solve_kernels(trace), trace_s
    assert _solve_kernels(_explain(gpu_ctx, batch, flags=api.FLAG_SHARED_DEVICE)[0]) == _solve_kernels(trace)
    assert _same_bits(out, shared)


# ---- 3b: a path alone in a one-path plan has the bits it has in the batch
@pytest.mark.parametrize("key", [("every", 4, "rest"), ("every", 2, "moving"), ("edge", u.LONGEST_ROWS, 4, "rest"),
                                 ("edge", u.LONGEST_ROWS, 2, "moving")], ids=u.key_id)
def test_a_path_alone_has_the_bits_it_has_in_the_batch(gpu_ctx, key):
    """alone: Smax = S (other record strides and offsets in LDS), wmax the path's own, one path per wavefront with its spare
    rows switched off.  A row's arithmetic reads only its own path's records and the steps beyond its nact are predicated off,
    so the bits are those inside the batch, at one and at two paths per wavefront"""
    ref = u.reference(key)
    batch, so = ref.batch, ref.batch.seg_offsets
    plain = gpu_ctx.solve_batch(batch, ref.times)
    shared = gpu_ctx.solve_batch(batch, ref.times, flags=api.FLAG_SHARED_DEVICE)
    assert _same_bits(plain, shared) and np.all(plain["status"] == 1)
    paths = range(0, batch.n_paths, 3) if key[0] == "every" else range(batch.n_paths)   # one path of every length | every path
    assert sorted({int(so[p + 1] - so[p]) for p in paths}) == sorted(set(np.diff(so).tolist()))
    differing = []
    for p in paths:
        a, b = int(so[p]), int(so[p + 1])
        alone, trace = _traced(gpu_ctx, batch.select([p]), ref.times[a:b])
        assert _solve_kernels(trace) == [ROWS], trace
        same = np.array_equal(alone["coeffs"], plain["coeffs"][a:b]) and alone["cost"][0] == plain["cost"][p] and alone["status"][0] == plain["status"][p]
        if not same:
            differing.append((p, b - a, util.coeff_error(alone["coeffs"], plain["coeffs"][a:b])))
    assert not differing, differing


# ---- 3c: the grouped dispatch
def _grouped(ctx, lengths, copies, n_batches):
    batches = [u.lengths_batch(lengths, copies, 4, 7_900_000 + 1000 * j) for j in range(n_batches)]
    times = [util.oracle_times(b) for b in batches]
    plan = api.Plan(ctx, batches[0].seg_offsets)
    opt = api.default_options(derivative_to_optimize=4)
    dbs, calls = [], []
    try:
        names = plan.explain(opt, n_batches)
        for b, t in zip(batches, times):
            assert np.array_equal(b.seg_offsets, batches[0].seg_offsets)
            db = api.DeviceBatch(b, "cuda:0")
            db.seg_times.copy_(torch.from_numpy(t))
            db.coeffs.fill_(NAN)
            db.cost.fill_(NAN)
            calls.append(plan.bind_solve(opt, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints))
            dbs.append(db)
        api.kernel_trace_reset()
        api.RoundRobin(calls, grouped=True)(n_batches)
        trace = api.kernel_trace()
        torch.cuda.synchronize()
        got = [{k: getattr(db, k).cpu().numpy() for k in ("coeffs", "cost", "status")} for db in dbs]
    finally:
        calls.clear()
        plan.close()
    return batches, times, got, trace, names


@pytest.mark.parametrize("lengths,copies,n_batches", [(lengths, 3, 3) for lengths in u.GROUP_LENGTHS] + [((89, 64, 2), 22, 16)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_grouped_dispatch_has_the_bits_of_the_single_launches(gpu_ctx, lengths, copies, n_batches):
    """batches of one plan with different waypoints in ONE dispatch.  Three batches of nine to twelve paths run one path per
    wavefront (79: the last below 64 KB; 80, 89, 179: the group kernel's own raise of the limit); sixteen batches of 66 paths are
    more than 1024 paths in the dispatch: two paths per wavefront, at 89 segments the last that fit"""
    batches, times, got, trace, names = _grouped(gpu_ctx, lengths, copies, n_batches)
    assert trace == [GROUP] and names == [GROUP], (trace, names)
    total = batches[0].n_paths * n_batches
    assert (total > 1024) == (n_batches == 16)
    for b, t, g in zip(batches, times, got):
        single, trace_1 = _traced(gpu_ctx, b, t)
        assert _solve_kernels(trace_1) == [ROWS], trace_1
        assert np.all(single["status"] == 1)
        assert _same_bits(g, single)
        if n_batches == 3:
            assert _same_bits(g, gpu_ctx.solve_batch(b, t, flags=api.FLAG_SHARED_DEVICE))


# ---- 4: the sampling tail at its edges
@pytest.mark.parametrize("key", u.TAIL_KEYS, ids=u.key_id)
def test_sampling_tail_at_its_size_edges(gpu_ctx, key):
    dt, cap = 0.2, 4096
    ref = u.reference(key)
    batch, so = ref.batch, ref.batch.seg_offsets
    Smax = int(np.diff(so).max())
    model = u.route(Smax, batch.n_paths, sampling=True)
    assert model["tail"] == (Smax <= 126) and model["raised"] == (Smax >= 55)
    out, trace = _traced(gpu_ctx, batch, ref.times, sampling_dt=dt, sample_capacity=cap)
    names, _ = _explain(gpu_ctx, batch, sampling_dt=dt, sample_capacity=cap)
    want = [ROWS_TAIL] if model["tail"] else [ROWS, SAMPLER]   # (the sampler's own launch is noted with its template argument)
    for noted in (trace, names):
        got = [SAMPLER if k.startswith(SAMPLER) else k for k in noted if k.startswith(("solve_", SAMPLER))]
        assert got == want, noted
    # the coefficients are those of the same call without sampling
    plain, trace_0 = _traced(gpu_ctx, batch, ref.times)
    assert _solve_kernels(trace_0) == [ROWS] and _same_bits(out, plain) and np.all(out["status"] == 1)
    _gates(u.key_id(key), want[0], ref, out)
    # the samples are plan.sample's on the returned coefficients and times
    plan = api.Plan(gpu_ctx, so)
    try:
        n_dev = torch.full((batch.n_paths,), -1, dtype=torch.int32, device="cuda")
        samples = torch.full((batch.n_paths, cap, 4), NAN, dtype=torch.float64, device="cuda")
        plan.sample(torch.from_numpy(out["coeffs"]).cuda(), torch.from_numpy(out["times"]).cuda(), dt, cap, n_dev, samples)
        torch.cuda.synchronize()
    finally:
        plan.close()
    separate, n_separate = samples.cpu().numpy(), n_dev.cpu().numpy()
    assert np.array_equal(out["n_samples"], n_separate), (out["n_samples"], n_separate)
    total = np.add.reduceat(ref.times, so[:-1])
    assert np.all(n_separate >= np.floor(total / dt)) and np.all(n_separate <= np.ceil(total / dt) + 1) and n_separate.max() <= cap
    for p in range(batch.n_paths):
        n = int(n_separate[p])
        assert np.array_equal(out["samples"][p, :n].view(np.uint64), separate[p, :n].view(np.uint64)), p
        assert np.all(np.isfinite(out["samples"][p, :n]))

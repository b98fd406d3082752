"""mrs_tg_plan_path_deviation / mrs_tg_plan_path_deviation_vjp on the GPU (path_deviation_kernel, path_deviation_vjp_kernel,
DESIGN.md section 11b) and autograd.path_deviation on top of them: the small shapes built to break the ballot rounds and the
chunk seam against the CPU harness bit for bit, whole batches against the oracle's scan bit for bit, NULL outputs, unwritten
neighbours, the chain solve -> sample -> path_deviation -> loss, determinism.  NaN inputs are ordinary data here (they fill
every row and column the kernels must not read): nothing provokes a fault."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd, problem as pr
from oracle import pyoracle as po
from tests import deviation_util as du

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL, ISENTINEL = -777.25, -7
FORWARD = ("deviation", "cursor", "max_deviation", "argmax", "segment_max")
BACKWARD = ("grad_samples", "grad_waypoints")


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)).cuda()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return du.build_harness(tmp_path_factory.mktemp("deviation_gpu"))


def _uniform(problems, first_segment=None, capacity=None):
    """copies of the problems with one first_segment and one capacity (what a call has one of), the upstream padded"""
    cap = max(p["capacity"] for p in problems) if capacity is None else capacity
    out = []
    for p in problems:
        g = np.full(cap, NAN)
        k = du.scanned_rows(p)
        g[:k] = p["upstream"][:k]
        # (a shape that claims more samples than it has rows is an overflow of ITS capacity: in a larger one it has its rows)
        out.append(dict(p, capacity=cap, upstream=g, n_samples=min(p["n_samples"], max(p["samples"].shape[0], p["capacity"])),
                        first_segment=p["first_segment"] if first_segment is None else first_segment))
    return out


def _guarded(rows, shape_tail, dtype, fill):
    """a tensor with one guard row in front and one behind, and the view between them that the call gets"""
    full = torch.full((rows + 2,) + tuple(shape_tail), fill, dtype=dtype, device="cuda")
    return full, full[1:rows + 1]


def _run(ctx, probs, want=FORWARD + BACKWARD):
    """one forward and one backward call on the problems as one batch (same capacity, same first_segment) -> host arrays by
    name, plus seg_offsets and the plan's order.  Every row, column and element the kernels must not read holds NaN; every
    output is prefilled with a sentinel and has guard rows on both sides, which are checked here."""
    P, cap, fs = len(probs), probs[0]["capacity"], probs[0]["first_segment"]
    assert all(p["capacity"] == cap and p["first_segment"] == fs for p in probs)
    S = np.array([p["waypoints"].shape[0] - 1 for p in probs])
    so = np.concatenate([[0], np.cumsum(S)]).astype(np.int32)
    nV = int(so[-1]) + P
    w4 = np.full((nV, 4), NAN)
    smp = np.full((P, cap, 4), NAN)
    g = np.full((P, cap), NAN)
    for q, p in enumerate(probs):
        w4[so[q] + q:so[q + 1] + q + 1, :3] = p["waypoints"]
        m = max(min(p["n_samples"], cap), 0)
        smp[q, :m, :3] = p["samples"][:m]
        g[q] = p["upstream"]
    n = _dev(np.array([p["n_samples"] for p in probs]), np.int32)
    status = _dev(np.array([p["status"] for p in probs]), np.int32)
    spec = dict(deviation=(P, (cap,), torch.float64, SENTINEL), cursor=(P, (cap,), torch.int32, ISENTINEL),
                max_deviation=(P, (), torch.float64, SENTINEL), argmax=(P, (), torch.int32, ISENTINEL),
                segment_max=(int(so[-1]), (), torch.float64, SENTINEL), grad_samples=(P, (cap, 4), torch.float64, SENTINEL),
                grad_waypoints=(nV, (4,), torch.float64, SENTINEL))
    full, view = {}, {}
    for name in want:
        full[name], view[name] = _guarded(*spec[name])
    plan = api.Plan(ctx, so)
    try:
        d_s, d_w, d_g = _dev(smp), _dev(w4), _dev(g)
        if any(k in want for k in FORWARD):
            plan.path_deviation(d_s, n, d_w, first_segment=bool(fs), status=status, **{k: view.get(k) for k in FORWARD})
        if any(k in want for k in BACKWARD):
            plan.path_deviation_vjp(d_s, n, d_w, d_g, status=status, **{k: view.get(k) for k in BACKWARD})
        torch.cuda.synchronize()
        order = np.array(plan.order)
    finally:
        plan.close()
    out = dict(seg_offsets=so, order=order)
    for name in want:
        host = full[name].cpu().numpy()
        fill = spec[name][3]
        assert np.all(host[0] == fill) and np.all(host[-1] == fill), "%s: a neighbour of the plan's rows was written" % name
        out[name] = host[1:-1]
    return out


def _compare(out, probs, cpu, want=FORWARD + BACKWARD):
    """every output of every path against the CPU harness, bit for bit; the rows behind the scan are zeros / -1"""
    so = out["seg_offsets"]
    for q, (p, h) in enumerate(zip(probs, cpu)):
        k = len(h["cursor"])          # scanned (0 for a path with status <= 0)
        kk = du.scanned_rows(p)
        a, b = int(so[q]), int(so[q + 1])
        tag = (q, p["n_samples"], p["capacity"], b - a)
        if "deviation" in want:
            assert du.same_bits(out["deviation"][q, :k], h["deviation"]), tag
            assert np.all(out["deviation"][q, k:] == 0.0), tag
        if "cursor" in want:
            assert np.array_equal(out["cursor"][q, :k], h["cursor"]) and np.all(out["cursor"][q, k:] == -1), tag
        if "max_deviation" in want:
            assert du.same_bits(out["max_deviation"][q], h["max_deviation"]), tag
        if "argmax" in want:
            assert out["argmax"][q] == h["argmax"], tag
        if "segment_max" in want:
            assert du.same_bits(out["segment_max"][a:b], h["segment_max"]), tag
        if "grad_samples" in want:
            gs = out["grad_samples"][q]
            assert du.same_bits(gs[:kk, :3], h["grad_samples"]), tag
            assert np.all(gs[:, 3] == 0.0) and np.all(gs[kk:] == 0.0), tag
        if "grad_waypoints" in want:
            gw = out["grad_waypoints"][a + q:b + q + 1]
            assert du.same_bits(gw[:, :3], h["grad_waypoints"]), tag
            assert np.all(gw[:, 3] == 0.0), tag


def test_the_library_reports_the_capability_and_times_both_kernels(gpu_ctx):
    assert api.CAP_DEVIATION == 128 and api.KERNEL_DEVIATION == 8 and api.KERNEL_DEVIATION_VJP == 9
    assert api.capabilities() & api.CAP_DEVIATION
    probs = _uniform(du.ragged_batch(6, 3), first_segment=1)
    try:
        gpu_ctx.set_profiling(True)
        _run(gpu_ctx, probs)
        assert gpu_ctx.last_kernel_ms(api.KERNEL_DEVIATION) > 0
        assert gpu_ctx.last_kernel_ms(api.KERNEL_DEVIATION_VJP) > 0
    finally:
        gpu_ctx.set_profiling(False)


def test_every_small_shape_alone_is_the_harness_in_bits(gpu_ctx, harness):
    """one plan per shape, with the shape's own capacity (n_samples = capacity + 1 among them) and first_segment"""
    shapes = du.small_shapes()
    cpu = du.run_harness(harness, list(shapes.values()))
    for (name, p), h in zip(shapes.items(), cpu):
        probs = _uniform([p])
        try:
            _compare(_run(gpu_ctx, probs), probs, [h])
        except AssertionError as e:
            raise AssertionError("shape %s: %s" % (name, e))


@pytest.mark.parametrize("first_segment", [0, 1])
def test_small_shapes_as_one_batch_with_a_dead_path_between(gpu_ctx, harness, first_segment):
    """all shapes in one call: 1 to 30 segments in the caller's order (the plan sorts them), a status-0 path between good
    ones whose samples are NaN, one capacity for all"""
    shapes = list(du.small_shapes().values())
    dead = dict(shapes[3], status=0, samples=np.full_like(shapes[3]["samples"], NAN))
    probs = _uniform(shapes[:5] + [dead] + shapes[5:], first_segment=first_segment)
    cpu = du.run_harness(harness, probs)
    out = _run(gpu_ctx, probs)
    assert not np.array_equal(out["order"], np.arange(len(probs)))   # the plan's order is not the caller's
    _compare(out, probs, cpu)
    assert np.all(out["deviation"][5] == 0.0) and np.all(out["cursor"][5] == -1) and np.all(out["grad_samples"][5] == 0.0)


def test_a_ragged_batch_in_an_order_the_plan_does_not_keep(gpu_ctx, harness):
    probs = _uniform(du.ragged_batch(40, 17), first_segment=0)
    S = [p["waypoints"].shape[0] - 1 for p in probs]
    assert min(S) >= 3 and max(S) <= 30 and S != sorted(S, reverse=True) and probs[1]["status"] == 0
    out = _run(gpu_ctx, probs)
    assert not np.array_equal(out["order"], np.arange(len(probs)))
    _compare(out, probs, du.run_harness(harness, probs))


def test_null_output_combinations_change_no_bit(gpu_ctx):
    probs = _uniform(du.ragged_batch(9, 23), first_segment=1)
    ref = _run(gpu_ctx, probs)
    combos = [(k,) for k in FORWARD + BACKWARD] + [("max_deviation", "argmax"), ("deviation", "segment_max"),
                                                   ("cursor", "segment_max", "grad_waypoints")]
    for want in combos:
        out = _run(gpu_ctx, probs, want=want)
        for k in want:
            assert np.array_equal(out[k], ref[k]) and (out[k].dtype != np.float64 or du.same_bits(out[k], ref[k])), want
    plan = api.Plan(gpu_ctx, ref["seg_offsets"])
    try:
        s = torch.zeros((9, 4, 4), dtype=torch.float64, device="cuda")
        n = torch.zeros(9, dtype=torch.int32, device="cuda")
        w = torch.zeros((int(ref["seg_offsets"][-1]) + 9, 4), dtype=torch.float64, device="cuda")
        with pytest.raises(api.MrsTgError):
            plan.path_deviation(s, n, w)
        with pytest.raises(api.MrsTgError):
            plan.path_deviation_vjp(s, n, w, torch.zeros((9, 4), dtype=torch.float64, device="cuda"))
        with pytest.raises(api.MrsTgError):
            plan.path_deviation(s, None, w, deviation=torch.zeros((9, 4), dtype=torch.float64, device="cuda"))
    finally:
        plan.close()


def test_two_calls_give_the_same_bits(gpu_ctx):
    probs = _uniform(du.ragged_batch(64, 29), first_segment=1)
    a, b = _run(gpu_ctx, probs), _run(gpu_ctx, probs)
    for k in FORWARD + BACKWARD:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("n_seg,paths,first_segment", [(10, 1024, 1), ("ragged", 256, 0)])
def test_whole_batches_are_the_oracles_scan_in_bits(gpu_ctx, n_seg, paths, first_segment):
    """fixed-times solves sampled at 0.2 s: for EVERY path the maximum, its index, the cursors, the deviations and the segment
    maxima are the oracle's scan of the same samples, bit for bit"""
    batch = pr.random_batch(paths, n_seg, seed0=91000)
    out = gpu_ctx.solve_batch(batch, None)   # the library's estimator, then the fixed-times solve
    assert np.all(out["status"] > 0)
    so = np.asarray(batch.seg_offsets, dtype=np.int64)
    dt = 0.2
    cap = int(np.max(np.add.reduceat(out["times"], so[:-1])) / dt) + 8
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        c, t, w = _dev(out["coeffs"]), _dev(out["times"]), _dev(batch.waypoints)
        n = torch.zeros(paths, dtype=torch.int32, device="cuda")
        samples = torch.zeros((paths, cap, 4), dtype=torch.float64, device="cuda")
        plan.sample(c, t, dt, cap, n, samples)
        dev = torch.full((paths, cap), SENTINEL, dtype=torch.float64, device="cuda")
        cur = torch.full((paths, cap), ISENTINEL, dtype=torch.int32, device="cuda")
        mx = torch.full((paths,), SENTINEL, dtype=torch.float64, device="cuda")
        arg = torch.full((paths,), ISENTINEL, dtype=torch.int32, device="cuda")
        seg = torch.full((batch.n_segments,), SENTINEL, dtype=torch.float64, device="cuda")
        plan.path_deviation(samples, n, w, first_segment=bool(first_segment), status=_dev(out["status"], np.int32),
                            deviation=dev, cursor=cur, max_deviation=mx, argmax=arg, segment_max=seg)
        torch.cuda.synchronize()
    finally:
        plan.close()
    n, smp = n.cpu().numpy(), samples.cpu().numpy()
    dev, cur, mx, arg, seg = (x.cpu().numpy() for x in (dev, cur, mx, arg, seg))
    assert np.all(n > 2) and np.all(n <= cap)
    scanned = advances = 0
    for p in range(paths):
        a, b = int(so[p]), int(so[p + 1])
        k = int(n[p]) - 1
        o = du.oracle_scan_rows(po, batch.waypoints[a + p:b + p + 1], smp[p], k, first_segment)
        assert np.array_equal(cur[p, :k], o["cursor"]) and np.all(cur[p, k:] == -1), p
        assert du.same_bits(dev[p, :k], o["deviation"]) and np.all(dev[p, k:] == 0.0), p
        assert du.same_bits(mx[p], o["max_deviation"]) and arg[p] == o["argmax"], p
        assert du.same_bits(seg[a:b], o["segment_max"]), p
        scanned += k
        advances += int(o["cursor"][-1])
    print("DEVIATION GPU vs ORACLE %s x %s: %d paths, %d scanned samples, %d cursor advances, all bits equal" %
          (paths, n_seg, paths, scanned, advances))
    assert advances >= paths


def test_chain_solve_sample_deviation_hinge_loss(gpu_ctx):
    """fixed_values.grad and seg_times.grad of a corridor loss through solve -> sample -> path_deviation, against the same
    chain whose deviation stage is a float64 torch restatement with the kernel's cursors.

    The bound.  The two chains share the solve and the sampler (same kernels, same bits); they differ in what the deviation
    stage hands back.  That is checked first, entry by entry: dL/dsamples and dL/dwaypoints of the kernel and of the restatement
    differ by at most the derived bound of tests/test_deviation_host.py -- 16 eps max(|p|, |a|, |b|) / d |g| of the sample for
    its own three entries, summed over the contributing samples for a waypoint's.  Every sample's own gradient has length |g|,
    so this is a relative error of at most rho = 16 eps max_i(max(|p|, |a|, |b|) / d_i) of every sample's contribution, and
    the final gradients are held to rho times the restatement's own gradient norm, per path: |fixed_values.grad difference|
    <= rho ||fixed_values.grad||_2, and the same for seg_times.grad.  (Measured on an MI355X: rho 4e-14 .. 5e-13, differences
    9e-14 .. 4e-13 on gradients of 2e+1 .. 8e+1.  A sharper, entry-wise form -- the stage bounds pushed through the linear
    backward pass one entry at a time, sum_e b_e |J^T 1_e| -- held on all but a few entries, where the rounding of the shared
    backward kernels themselves, which that form leaves out, added 9e-15: two units in the last place of the gradient.)"""
    batch = du.chain_batch()
    cap, dt, h = du.CHAIN_CAPACITY, du.CHAIN_DT, du.CHAIN_CORRIDOR
    times0 = gpu_ctx.solve_batch(batch, None)["times"]
    so = np.asarray(batch.seg_offsets, dtype=np.int64)
    P = batch.n_paths
    v0 = so[:-1] + np.arange(P)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    mask = _dev(batch.fixed_mask)
    try:
        def chain(stage):
            fv = _dev(batch.fixed_values).requires_grad_(True)
            times = _dev(times0).requires_grad_(True)
            coeffs, _, status = autograd.solve(plan, mask, fv, times)
            samples, n = autograd.sample(plan, coeffs, times, dt, cap, status)
            wp = fv[:, 0, :]
            samples.retain_grad()
            wp.retain_grad()
            d, cursor = stage(samples, n, wp, status)
            loss = (torch.relu(d - h) * (cursor > 0)).sum()
            return dict(fv=fv, times=times, samples=samples, wp=wp, n=n, status=status, d=d, cursor=cursor, loss=loss)

        k = chain(lambda s, n, w, st: autograd.path_deviation(plan, s, n, w, first_segment=False, status=st))
        assert not k["cursor"].requires_grad and k["d"].requires_grad
        cursor = k["cursor"]
        r = chain(lambda s, n, w, st: (du.torch_deviation(torch, s, w, cursor, _dev(v0)), cursor))
        k["loss"].backward()
        r["loss"].backward()
        torch.cuda.synchronize()
        assert bool(torch.all(k["status"] > 0)) and bool(torch.all(k["n"] == cap + 1))
        # forward: the restatement agrees with the kernel to rounding, the loss is alive on every path
        dk, dr, cur = k["d"].detach().cpu().numpy(), r["d"].detach().cpu().numpy(), cursor.cpu().numpy()
        assert np.max(np.abs(dk - dr)) <= 1e-12
        counted = cur > 0
        active = counted & (dk > h)
        assert np.all(cur[:, :cap - 1] >= 0) and np.all(cur[:, cap - 1:] == -1)
        assert np.all(dk[counted] >= 1e-3) and np.all(active.sum(axis=1) >= 10)
        # the stage's own gradients, entry by entry, within the derived bound
        smp, wp4 = k["samples"].detach().cpu().numpy(), batch.fixed_values[:, 0, :]
        Gs_k, Gs_r = k["samples"].grad.cpu().numpy(), r["samples"].grad.cpu().numpy()
        Gw_k, Gw_r = k["wp"].grad.cpu().numpy(), r["wp"].grad.cpu().numpy()
        rho = np.zeros(P)
        for p in range(P):
            w = wp4[v0[p]:v0[p] + 5]
            b = du.stage_bound(smp[p, :cap - 1], w, cur[p, :cap - 1], dk[p, :cap - 1], active[p, :cap - 1].astype(np.float64))
            rho[p] = b.max()
            assert np.all(np.abs(Gs_k[p, :cap - 1, :3] - Gs_r[p, :cap - 1, :3]) <= b[:, None]), p
            bw = np.zeros(5)
            for i, c in enumerate(cur[p, :cap - 1]):
                bw[c] += b[i]
                bw[c + 1] += b[i]
            assert np.all(np.abs(Gw_k[v0[p]:v0[p] + 5, :3] - Gw_r[v0[p]:v0[p] + 5, :3]) <= bw[:, None]), p
            assert np.all(Gs_k[p, :, 3] == 0.0) and np.all(Gw_k[v0[p]:v0[p] + 5, 3] == 0.0)
        gpu_ctx.use_torch_stream()
    finally:
        plan.close()
    gfk, gfr, gtk, gtr = (x.grad.cpu().numpy() for x in (k["fv"], r["fv"], k["times"], r["times"]))
    worst = []
    for p in range(P):
        vs, ss = slice(v0[p], v0[p] + 5), slice(so[p], so[p + 1])
        ef, et = np.abs(gfk[vs] - gfr[vs]).max(), np.abs(gtk[ss] - gtr[ss]).max()
        nf, nt = np.linalg.norm(gfr[vs]), np.linalg.norm(gtr[ss])
        print("DEVIATION GPU CHAIN path %d: rho %.2e; fixed_values.grad max |diff| %.2e (bound %.2e, ||grad|| %.2e); "
              "seg_times.grad max |diff| %.2e (bound %.2e, ||grad|| %.2e)" % (p, rho[p], ef, rho[p] * nf, nf, et, rho[p] * nt, nt))
        assert nf > 0 and nt > 0
        worst.append((ef - rho[p] * nf, et - rho[p] * nt))
    assert all(f <= 0.0 and t <= 0.0 for f, t in worst), worst

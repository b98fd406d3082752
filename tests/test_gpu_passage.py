"""mrs_tg_plan_waypoint_passage / mrs_tg_plan_waypoint_passage_vjp on the GPU (waypoint_passage_kernel,
waypoint_passage_vjp_kernel) and autograd.waypoint_passage on top of them: the small shapes built to
break the ballot rounds and the chunk seam against the CPU harness bit for bit, requested waypoints that are not the plan's
vertices, whole batches against the oracle's scan bit for bit, NULL outputs, unwritten neighbours, the chain solve -> sample ->
waypoint_passage -> loss, determinism.  NaN inputs are ordinary data here (they fill every row, column and upstream entry the
kernels must not read): nothing provokes a fault."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd, problem as pr
from oracle import pyoracle as po
from tests import deviation_util as du
from tests import passage_util as pu

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL, ISENTINEL = -777.25, -7
FORWARD = ("index", "count", "miss", "fraction")
BACKWARD = ("grad_samples", "grad_waypoints")


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)).cuda()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return pu.build_harness(tmp_path_factory.mktemp("passage_gpu"))


def _uniform(problems, capacity=None):
    """copies of the problems with one capacity (what a call has one of)"""
    cap = max(p["capacity"] for p in problems) if capacity is None else capacity
    # (a shape that claims more samples than it has rows is an overflow of ITS capacity: in a larger one it has its rows)
    return [dict(p, capacity=cap, n_samples=min(p["n_samples"], max(p["samples"].shape[0], p["capacity"]))) for p in problems]


def _guarded(rows, shape_tail, dtype, fill):
    """a tensor with one guard row in front and one behind, and the view between them that the call gets"""
    full = torch.full((rows + 2,) + tuple(shape_tail), fill, dtype=dtype, device="cuda")
    return full, full[1:rows + 1]


def _run(ctx, probs, cpu, segments=None, offsets=True, want=FORWARD + BACKWARD):
    """one forward and one backward call on the problems as one batch (same capacity) -> host arrays by name, plus wp_offsets
    and the plan's order.  segments: the segment counts of the plan's paths (with offsets they are free: the plan gives the
    order of the paths only; without, path q has segments[q] + 1 waypoints).  Every row, column and element the kernels must
    not read holds NaN -- the upstreams of the waypoints that cpu (the harness) finds unreached among them; every output is
    prefilled with a sentinel and has guard rows on both sides, which are checked here."""
    P, cap = len(probs), probs[0]["capacity"]
    assert all(p["capacity"] == cap for p in probs)
    W = np.array([len(p["waypoints"]) for p in probs])
    S = np.array([1 + (5 * q) % 7 for q in range(P)] if segments is None else segments)
    assert offsets or np.array_equal(S + 1, W)
    so = np.concatenate([[0], np.cumsum(S)]).astype(np.int32)
    wo = np.concatenate([[0], np.cumsum(W)]).astype(np.int32)
    nW = int(wo[-1])
    w4 = np.full((nW + 1, 4), NAN)   # (a row behind the last path's, never read: a batch without any waypoint has an array)
    smp = np.full((P, cap, 4), NAN)
    gm, gt = np.full(nW, NAN), np.full(nW, NAN)
    for q, (p, h) in enumerate(zip(probs, cpu)):
        w4[wo[q]:wo[q + 1], :3] = p["waypoints"]
        m = pu.rows(p)
        smp[q, :m, :3] = p["samples"][:m]
        k = h["count"]
        gm[wo[q]:wo[q] + k], gt[wo[q]:wo[q] + k] = p["grad_miss"][:k], p["grad_fraction"][:k]
    n = _dev(np.array([p["n_samples"] for p in probs]), np.int32)
    status = _dev(np.array([p["status"] for p in probs]), np.int32)
    spec = dict(index=(nW, (), torch.int32, ISENTINEL), count=(P, (), torch.int32, ISENTINEL),
                miss=(nW, (), torch.float64, SENTINEL), fraction=(nW, (), torch.float64, SENTINEL),
                grad_samples=(P, (cap, 4), torch.float64, SENTINEL), grad_waypoints=(nW, (4,), torch.float64, SENTINEL))
    full, view = {}, {}
    for name in want:
        full[name], view[name] = _guarded(*spec[name])
    plan = api.Plan(ctx, so)
    try:
        d_s, d_w, d_o = _dev(smp), _dev(w4), (_dev(wo) if offsets else None)
        if any(k in want for k in FORWARD):
            plan.waypoint_passage(d_s, n, d_w, wp_offsets=d_o, status=status, **{k: view.get(k) for k in FORWARD})
        if any(k in want for k in BACKWARD):
            plan.waypoint_passage_vjp(d_s, n, d_w, grad_miss=_dev(gm), grad_fraction=_dev(gt), wp_offsets=d_o, status=status,
                                      **{k: view.get(k) for k in BACKWARD})
        torch.cuda.synchronize()
        order = np.array(plan.order)
    finally:
        plan.close()
    out = dict(wp_offsets=wo, order=order)
    for name in want:
        host = full[name].cpu().numpy()
        fill = spec[name][3]
        assert np.all(host[0] == fill) and np.all(host[-1] == fill), "%s: a neighbour of the plan's rows was written" % name
        out[name] = host[1:-1]
    return out


def _compare(out, probs, cpu, want=FORWARD + BACKWARD):
    """every output of every path against the CPU harness, bit for bit"""
    wo = out["wp_offsets"]
    for q, (p, h) in enumerate(zip(probs, cpu)):
        a, b = int(wo[q]), int(wo[q + 1])
        m = pu.rows(p)
        tag = (q, p["n_samples"], p["capacity"], b - a)
        if "index" in want:
            assert np.array_equal(out["index"][a:b], h["index"]), tag
        if "count" in want:
            assert out["count"][q] == h["count"], tag
        if "miss" in want:
            assert pu.same_bits(out["miss"][a:b], h["miss"]), tag
        if "fraction" in want:
            assert pu.same_bits(out["fraction"][a:b], h["fraction"]), tag
        if "grad_samples" in want:
            gs = out["grad_samples"][q]
            assert pu.same_bits(gs[:m, :3], h["grad_samples"]), tag
            assert np.all(gs[:, 3] == 0.0) and np.all(gs[m:] == 0.0), tag
        if "grad_waypoints" in want:
            gw = out["grad_waypoints"][a:b]
            assert pu.same_bits(gw[:, :3], h["grad_waypoints"]), tag
            assert np.all(gw[:, 3] == 0.0), tag


def test_the_library_reports_the_capability_and_traces_both_kernels(gpu_ctx, harness):
    assert api.CAP_WAYPOINT_PASSAGE == 512 and api.KERNEL_PASSAGE == 12 and api.KERNEL_PASSAGE_VJP == 13
    assert api.capabilities() & api.CAP_WAYPOINT_PASSAGE
    probs = _uniform(pu.ragged_batch(6, 3)[0])
    cpu = pu.run_harness(harness, probs)
    try:
        gpu_ctx.set_profiling(True)
        api.kernel_trace_reset()
        _run(gpu_ctx, probs, cpu)
        trace = api.kernel_trace()
        assert "waypoint_passage_kernel" in trace and "waypoint_passage_vjp_kernel" in trace, trace
        assert gpu_ctx.last_kernel_ms(api.KERNEL_PASSAGE) > 0
        assert gpu_ctx.last_kernel_ms(api.KERNEL_PASSAGE_VJP) > 0
    finally:
        gpu_ctx.set_profiling(False)


def test_every_small_shape_alone_is_the_harness_in_bits(gpu_ctx, harness):
    """one plan per shape, with the shape's own capacity (n_samples = capacity + 1 among them); W = 0 travels through wp_offsets"""
    shapes = pu.small_shapes()
    cpu = pu.run_harness(harness, list(shapes.values()))
    for (name, p), h in zip(shapes.items(), cpu):
        try:
            _compare(_run(gpu_ctx, [p], [h]), [p], [h])
        except AssertionError as e:
            raise AssertionError("shape %s: %s" % (name, e))


def test_small_shapes_as_one_batch_with_a_dead_path_between(gpu_ctx, harness):
    """all shapes in one call, in an order the plan does not keep, a status-0 path between good ones whose samples are NaN,
    one capacity for all"""
    shapes = list(pu.small_shapes().values())
    dead = dict(shapes[3], status=0, samples=np.full_like(shapes[3]["samples"], NAN))
    probs = _uniform(shapes[:5] + [dead] + shapes[5:])
    cpu = pu.run_harness(harness, probs)
    out = _run(gpu_ctx, probs, cpu)
    assert not np.array_equal(out["order"], np.arange(len(probs)))   # the plan's order is not the caller's
    _compare(out, probs, cpu)
    a, b = out["wp_offsets"][5:7]
    assert out["count"][5] == 0 and np.all(out["index"][a:b] == -1) and np.all(out["miss"][a:b] == 0.0)
    assert np.all(out["grad_samples"][5] == 0.0) and np.all(out["grad_waypoints"][a:b] == 0.0)


@pytest.mark.parametrize("every,extra", [(2, 0), (1, 3)])
def test_requested_waypoints_that_are_not_the_plans_vertices(gpu_ctx, harness, every, extra):
    """a ragged batch whose requested waypoints are every second vertex of the plan's paths, and one whose requested waypoints
    are the vertices plus points off the path (those near enough are passed, the first one that is not ends the path's list);
    the paths in an order the plan does not keep"""
    probs, S = pu.ragged_batch(40, 17, every=every, extra=extra)
    probs = _uniform(probs)
    assert min(S) >= 3 and max(S) <= 30 and S != sorted(S, reverse=True) and probs[1]["status"] == 0
    W = [len(p["waypoints"]) for p in probs]
    assert W == [(s + 2) // 2 if every == 2 else s + 1 + extra for s in S]
    cpu = pu.run_harness(harness, probs)
    reached = sum(h["count"] for h in cpu)
    assert reached >= 100 and (extra == 0 or any(0 < h["count"] < w for h, w in zip(cpu, W)))
    out = _run(gpu_ctx, probs, cpu, segments=S)
    assert not np.array_equal(out["order"], np.arange(len(probs)))
    _compare(out, probs, cpu)


def test_no_offsets_means_the_plans_vertices_in_the_same_bits(gpu_ctx, harness):
    probs, S = pu.ragged_batch(40, 19)
    probs = _uniform(probs)
    cpu = pu.run_harness(harness, probs)
    given = _run(gpu_ctx, probs, cpu, segments=S, offsets=True)
    own = _run(gpu_ctx, probs, cpu, segments=S, offsets=False)
    _compare(own, probs, cpu)
    for k in FORWARD + BACKWARD:
        assert given[k].tobytes() == own[k].tobytes(), k


def test_null_output_combinations_change_no_bit(gpu_ctx, harness):
    probs, S = pu.ragged_batch(9, 23, extra=2)
    probs = _uniform(probs)
    cpu = pu.run_harness(harness, probs)
    ref = _run(gpu_ctx, probs, cpu, segments=S)
    # every non-empty choice of the forward's four outputs and of the backward's two
    combos = [tuple(k for b, k in enumerate(names) if bits >> b & 1) for names in (FORWARD, BACKWARD)
              for bits in range(1, 1 << len(names))]
    assert len(combos) == 15 + 3
    for want in combos:
        out = _run(gpu_ctx, probs, cpu, segments=S, want=want)
        for k in want:
            assert out[k].tobytes() == ref[k].tobytes(), want
    # either upstream may be NULL, which counts as zero
    zero = [dict(p, grad_fraction=np.zeros_like(p["grad_fraction"])) for p in probs]
    cpu_m = pu.run_harness(harness, zero)
    so = np.concatenate([[0], np.cumsum(S)]).astype(np.int32)
    wo = ref["wp_offsets"]
    plan = api.Plan(gpu_ctx, so)
    try:
        P, cap, nW = len(probs), probs[0]["capacity"], int(wo[-1])
        smp, w4, gm = np.zeros((P, cap, 4)), np.zeros((nW, 4)), np.zeros(nW)
        for q, p in enumerate(probs):
            smp[q, :pu.rows(p), :3] = p["samples"][:pu.rows(p)]
            w4[wo[q]:wo[q + 1], :3] = p["waypoints"]
            gm[wo[q]:wo[q + 1]] = p["grad_miss"]
        s, w, n = _dev(smp), _dev(w4), _dev(np.array([p["n_samples"] for p in probs]), np.int32)
        st, off = _dev(np.array([p["status"] for p in probs]), np.int32), _dev(wo)
        gs = torch.full((P, cap, 4), SENTINEL, dtype=torch.float64, device="cuda")
        gw = torch.full((nW, 4), SENTINEL, dtype=torch.float64, device="cuda")
        plan.waypoint_passage_vjp(s, n, w, grad_miss=_dev(gm), grad_fraction=None, wp_offsets=off, status=st, grad_samples=gs,
                                  grad_waypoints=gw)
        torch.cuda.synchronize()
        _compare(dict(wp_offsets=wo, grad_samples=gs.cpu().numpy(), grad_waypoints=gw.cpu().numpy()), probs, cpu_m, want=BACKWARD)
        with pytest.raises(api.MrsTgError):
            plan.waypoint_passage(s, n, w, wp_offsets=off)
        with pytest.raises(api.MrsTgError):
            plan.waypoint_passage_vjp(s, n, w, grad_miss=_dev(gm), wp_offsets=off)
        with pytest.raises(api.MrsTgError):
            plan.waypoint_passage(s, None, w, wp_offsets=off, count=torch.zeros(P, dtype=torch.int32, device="cuda"))
    finally:
        plan.close()


def test_two_calls_give_the_same_bits(gpu_ctx, harness):
    probs, S = pu.ragged_batch(64, 29, extra=1)
    probs = _uniform(probs)
    cpu = pu.run_harness(harness, probs)
    a, b = _run(gpu_ctx, probs, cpu, segments=S), _run(gpu_ctx, probs, cpu, segments=S)
    for k in FORWARD + BACKWARD:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("n_seg,paths", [(10, 1024), ("ragged", 256)])
def test_whole_batches_are_the_oracles_scan_in_bits(gpu_ctx, n_seg, paths):
    """the library's estimator and fixed-times solve sampled at 0.2 s: for EVERY path index and count are
    mto_waypoint_trajectory_idxs on the same samples and api.waypoint_trajectory_idxs, and miss is mto_dist_from_segment in
    bits; every path reaches at least W - 1 of its waypoints and the batch at least 99 % of all of them"""
    batch = pr.random_batch(paths, n_seg, seed0=93000)
    out = gpu_ctx.solve_batch(batch, None)
    assert np.all(out["status"] > 0)
    so = np.asarray(batch.seg_offsets, dtype=np.int64)
    dt = 0.2
    cap = int(np.max(np.add.reduceat(out["times"], so[:-1])) / dt) + 8
    nV = batch.n_segments + paths
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        c, t, w = _dev(out["coeffs"]), _dev(out["times"]), _dev(batch.waypoints)
        n = torch.zeros(paths, dtype=torch.int32, device="cuda")
        samples = torch.zeros((paths, cap, 4), dtype=torch.float64, device="cuda")
        plan.sample(c, t, dt, cap, n, samples)
        index = torch.full((nV,), ISENTINEL, dtype=torch.int32, device="cuda")
        count = torch.full((paths,), ISENTINEL, dtype=torch.int32, device="cuda")
        miss = torch.full((nV,), SENTINEL, dtype=torch.float64, device="cuda")
        fraction = torch.full((nV,), SENTINEL, dtype=torch.float64, device="cuda")
        plan.waypoint_passage(samples, n, w, status=_dev(out["status"], np.int32), index=index, count=count, miss=miss,
                              fraction=fraction)
        torch.cuda.synchronize()
    finally:
        plan.close()
    n, smp = n.cpu().numpy(), samples.cpu().numpy()
    index, count, miss, fraction = (x.cpu().numpy() for x in (index, count, miss, fraction))
    assert np.all(n > 2) and np.all(n <= cap)
    reached = adjacent = 0
    for p in range(paths):
        a, b = int(so[p]) + p, int(so[p + 1]) + p + 1
        o = pu.oracle_scan_rows(po, batch.waypoints[a:b], smp[p], int(n[p]))
        k = o["count"]
        assert count[p] == k and np.array_equal(index[a:b], o["index"]), p
        assert pu.same_bits(miss[a:b], o["miss"]), p
        assert api.waypoint_trajectory_idxs(smp[p, :n[p]], batch.waypoints[a:b]).tolist() == index[a:a + k].tolist(), p
        assert np.all((fraction[a:a + k] >= 0.0) & (fraction[a:a + k] <= 1.0)) and np.all(fraction[a + k:b] == 0.0), p
        assert k >= b - a - 1, (p, k, b - a)
        reached += k
        adjacent += int(np.sum(np.diff(index[a:a + k]) == 1))
    print("PASSAGE GPU vs ORACLE %s x %s: %d paths, %d of %d waypoints reached, at most %d samples per path, %d pairs of hits "
          "on adjacent steps, all bits equal" % (paths, n_seg, paths, reached, nV, n.max(), adjacent))
    assert reached >= 0.99 * nV


def test_chain_solve_sample_passage_arrival_loss(gpu_ctx):
    """fixed_values.grad and seg_times.grad of sum_k ((index + fraction) dt - target_k)^2 + sum_k miss_k^2 through
    solve -> sample -> waypoint_passage, the requested waypoints being the vertices moved 2 to 5 cm off the path
    (pu.chain_request), against the same chain whose last stage is a float64 torch restatement with the kernel's indices.

    The bound.  The two chains share the solve and the sampler (same kernels, same bits); they differ in what the last stage
    hands back.  That is checked first, entry by entry: dL/dsamples and dL/dwaypoints of the kernel and of the restatement differ
    by at most the two derived bounds of tests/test_passage_host.py per hit -- 16 eps max(|p|, |a|, |b|) / m |g_m| for the miss
    and, for an interior hit, 40 eps (1 + |q| / len) / len |g_t| for the fraction -- summed over the one or two hits a row takes
    part in.  A hit's miss rows have length |g_m| and its fraction rows at least |g_t| / len, so this is a relative error of at
    most rho = max over the hits of max(16 eps max(|p|, |a|, |b|) / m, 40 eps (1 + |q| / len)) of every hit's contribution, and
    the final gradients are held to rho times the restatement's own gradient norm, per path: |fixed_values.grad difference| <=
    rho ||fixed_values.grad||_2, and the same for seg_times.grad -- the argument of
    test_gpu_deviation.py::test_chain_solve_sample_deviation_hinge_loss.  The measured rho and differences are printed.
    (Measured on an MI355X: the stage's dL/dsamples differ by 2e-16 .. 7e-16, at most 0.012 of their bound; rho 8e-13 .. 4e-12;
    fixed_values.grad differs by 2e-15 .. 2e-14 against bounds of 3e-13 .. 7e-13 on gradients of norm 0.19 .. 0.36,
    seg_times.grad by 3e-15 .. 4e-14 against 4e-13 .. 3e-12 on norms 0.48 .. 0.95.)"""
    batch = du.chain_batch()
    cap, dt = pu.CHAIN_CAPACITY, du.CHAIN_DT
    times0 = gpu_ctx.solve_batch(batch, None)["times"]
    so = np.asarray(batch.seg_offsets, dtype=np.int64)
    P = batch.n_paths
    v0 = so[:-1] + np.arange(P)
    req0 = pu.chain_request(batch)
    path_of_wp = _dev(np.repeat(np.arange(P), 5))
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    mask = _dev(batch.fixed_mask)
    try:
        def chain(stage, index=None):
            fv = _dev(batch.fixed_values).requires_grad_(True)
            times = _dev(times0).requires_grad_(True)
            req = _dev(req0).requires_grad_(True)
            coeffs, _, status = autograd.solve(plan, mask, fv, times)
            samples, n = autograd.sample(plan, coeffs, times, dt, cap, status)
            samples.retain_grad()
            idx, miss, tau = stage(samples, n, req, status)
            reached = idx >= 0
            k = torch.arange(idx.shape[0], device=idx.device)
            target = (idx.double() + 0.25) * dt + 0.1 * (k % 3).double()   # a constant: the kernel's indices in both chains
            arrival = (idx.double() + tau) * dt
            loss = (((arrival - target) ** 2 + miss ** 2) * reached).sum()
            return dict(fv=fv, times=times, req=req, samples=samples, n=n, status=status, index=idx, miss=miss, tau=tau, loss=loss)

        def kernel_stage(s, n, w, st):
            index, count, miss, tau = autograd.waypoint_passage(plan, s, n, w, status=st)
            assert not index.requires_grad and not count.requires_grad and miss.requires_grad and tau.requires_grad
            return index, miss, tau

        k = chain(kernel_stage)
        index = k["index"]
        r = chain(lambda s, n, w, st: (index,) + pu.torch_passage(torch, s, w, index, path_of_wp))
        k["loss"].backward()
        r["loss"].backward()
        torch.cuda.synchronize()
        assert bool(torch.all(k["status"] > 0)) and bool(torch.all(k["n"] < cap))
        idx = index.cpu().numpy()
        mk, mr, tk, tr = (x.detach().cpu().numpy() for x in (k["miss"], r["miss"], k["tau"], r["tau"]))
        assert np.all(idx >= 0) and np.all(np.diff(idx.reshape(P, 5), axis=1) > 0)   # every waypoint is reached
        assert np.max(np.abs(mk - mr)) <= 1e-12 and np.max(np.abs(tk - tr)) <= 1e-9 and np.all(mk >= 1e-3)
        # the stage's own gradients, entry by entry, within the two derived bounds
        smp = k["samples"].detach().cpu().numpy()
        Gs_k, Gs_r = k["samples"].grad.cpu().numpy(), r["samples"].grad.cpu().numpy()
        Gw_k, Gw_r = k["req"].grad.cpu().numpy(), r["req"].grad.cpu().numpy()
        rho = np.zeros(P)
        for p in range(P):
            bs = np.zeros(cap)
            interior = 0
            for j in range(5):
                e = 5 * p + j
                i = idx[e]
                w, a, b = req0[e, :3], smp[p, i, :3], smp[p, i + 1, :3]
                g_m = 2.0 * mk[e]
                g_t = 2.0 * ((idx[e] + tk[e]) * dt - ((idx[e] + 0.25) * dt + 0.1 * (e % 3))) * dt
                inner = 0.0 < tk[e] < 1.0
                interior += int(inner)
                bound = pu.miss_bound(w, a, b, mk[e], g_m) + (pu.fraction_bound(w, a, b, g_t) if inner else 0.0)
                rho[p] = max(rho[p], pu.miss_bound(w, a, b, mk[e], 1.0), pu.fraction_bound(w, a, b, 1.0) * np.linalg.norm(b - a) if inner else 0.0)
                bs[i] += bound
                bs[i + 1] += bound
                assert np.all(np.abs(Gw_k[e, :3] - Gw_r[e, :3]) <= bound), (p, j, np.abs(Gw_k[e, :3] - Gw_r[e, :3]).max(), bound)
                assert np.any(Gw_k[e, :3] != 0.0) and Gw_k[e, 3] == 0.0
            assert interior >= 2, (p, interior)
            es = np.abs(Gs_k[p, :, :3] - Gs_r[p, :, :3]).max(axis=1)
            assert np.all(es <= bs), (p, float(np.max(es - bs)))
            print("PASSAGE GPU CHAIN path %d stage: dL/dsamples max |diff| %.2e, largest share of its bound %.3f" %
                  (p, es.max(), np.max(es[bs > 0] / bs[bs > 0])))
            assert np.all(Gs_k[p, :, 3] == 0.0)
        gpu_ctx.use_torch_stream()
    finally:
        plan.close()
    gfk, gfr, gtk, gtr = (x.grad.cpu().numpy() for x in (k["fv"], r["fv"], k["times"], r["times"]))
    worst = []
    for p in range(P):
        vs, ss = slice(v0[p], v0[p] + 5), slice(so[p], so[p + 1])
        ef, et = np.abs(gfk[vs] - gfr[vs]).max(), np.abs(gtk[ss] - gtr[ss]).max()
        nf, nt = np.linalg.norm(gfr[vs]), np.linalg.norm(gtr[ss])
        print("PASSAGE GPU CHAIN path %d: rho %.2e; fixed_values.grad max |diff| %.2e (bound %.2e, ||grad|| %.2e); "
              "seg_times.grad max |diff| %.2e (bound %.2e, ||grad|| %.2e)" % (p, rho[p], ef, rho[p] * nf, nf, et, rho[p] * nt, nt))
        assert nf > 0 and nt > 0
        worst.append((ef - rho[p] * nf, et - rho[p] * nt))
    assert all(f <= 0.0 and t <= 0.0 for f, t in worst), worst

"""mrs_tg_plan_initial_condition, mrs_tg_plan_prepend_initial_condition, mrs_tg_plan_splice_prediction and their backward passes
on the GPU (mrs_tg_initial.hip), with the autograd functions on top of them.  Everything these steps
produce is a copy of an input (but z + takeoff_height), so every comparison is bit for bit: the branch table against
api.prepare_initial_condition, the edit against a numpy restatement, the splice against api.splice_prediction on the grid of
sample and prefix rows around the chunk of 64, the backward passes against torch's autograd on index restatements, and the chain
initial_condition -> prepend -> solve -> sample -> splice -> loss against the same chain with the new backward passes called by
hand.  P <= 32 paths and a prediction capacity of 160 throughout."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api
from mrs_uav_trajectory_generation_amd import autograd as ag
from tests import initial_util as iu

pytestmark = pytest.mark.gpu
PRED_CAP = 160
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _count_plan(ctx, P):
    """the plan of a step that takes its path count and its context from it"""
    return api.Plan(ctx, np.arange(P + 1, dtype=np.int32))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _prediction_batch(rng, P):
    """four arrays [P][PRED_CAP][4], every element distinct"""
    return [rng.uniform(-50.0, 50.0, (P, PRED_CAP, 4)) for _ in range(4)]


def test_capability_bit_and_abi_version():
    assert api.capabilities() & api.CAP_INITIAL_CONDITION and api.CAP_INITIAL_CONDITION == 16384
    assert api.load_library().mrs_tg_abi_version() == 5
    assert (api.IC_PREPEND, api.IC_FROM_FUTURE, api.IC_DROP_FIRST, api.IC_FROM_TRACKER, api.IC_FROM_UAV, api.IC_FROM_PREDICTION,
            api.IC_INVALID) == (1, 2, 4, 8, 16, 32, 64)


def _run_initial_condition(ctx, rows, rng, takeoff=1.5):
    P = len(rows)
    pred = _prediction_batch(rng, P)
    tracker = rng.uniform(-5.0, 5.0, (P, 4, 4))
    uav = rng.uniform(-5.0, 5.0, (P, 4))
    flags = np.array([r["tracker"] * iu.FLAG_TRACKER | r["uav"] * iu.FLAG_UAV | r["dont"] * iu.FLAG_DONT_PREPEND for r in rows],
                     dtype=np.int32)
    vo = np.concatenate([[0], np.cumsum([r["n_wp"] for r in rows])]).astype(np.int32)
    decision = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    k = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    initial = torch.full((P, 4, 4), float("nan"), dtype=torch.float64, device=DEV)
    plan = _count_plan(ctx, P)
    try:
        plan.initial_condition(_dev(flags), _dev(tracker), _dev(np.array([r["age"] for r in rows])), _dev(uav), takeoff,
                               _dev(np.array([r["offset"] for r in rows])), _dev(vo), [_dev(a) for a in pred],
                               _dev(np.array([r["n_pred"] for r in rows], dtype=np.int32)), decision, k, initial)
        ctx.synchronize()
    finally:
        plan.close()
    return pred, tracker, uav, decision.cpu().numpy(), k.cpu().numpy(), initial.cpu().numpy()


def test_branch_table_against_prepare_initial_condition(gpu_ctx):
    rng = np.random.default_rng(11)
    table = iu.branch_table()
    table = [table[i] for i in rng.permutation(len(table))]      # a batch mixes the cases
    kinds = set()
    for b0 in range(0, len(table), 32):
        rows = table[b0:b0 + 32]
        pred, tracker, uav, decision, k, initial = _run_initial_condition(gpu_ctx, rows, rng)
        batch_kinds = set()
        for p, r in enumerate(rows):
            tr = dict(position=tracker[p, 0], velocity=tracker[p, 1], acceleration=tracker[p, 2], jerk=tracker[p, 3]) if r["tracker"] else None
            pr = dict(position=pred[0][p, :r["n_pred"]], velocity=pred[1][p, :r["n_pred"]], acceleration=pred[2][p, :r["n_pred"]],
                      jerk=pred[3][p, :r["n_pred"]]) if r["n_pred"] else None
            want = api.prepare_initial_condition(tr, r["age"], pr, uav[p] if r["uav"] else None, 1.5, r["offset"], r["n_wp"],
                                                 bool(r["dont"]))
            source = 0
            block = np.zeros((4, 4))
            if want["has_initial_condition"]:
                st = want["initial_state"]
                block = np.array([want["waypoint"], st["velocity"], st["acceleration"], st["jerk"]])
                assert st["heading"] == want["waypoint"][3]
                source = iu.FROM_PREDICTION if want["from_future"] else (iu.FROM_TRACKER if tr is not None and r["age"] <= 1.0 else iu.FROM_UAV)
            word = iu.expected_word(want["has_initial_condition"], want["from_future"], want["drop_first_waypoint"], source)
            assert decision[p] == word and k[p] == want["sample_offset"], (r, decision[p], word, k[p], want["sample_offset"])
            assert _bits(initial[p]) == _bits(block), (r, initial[p], block)
            batch_kinds.add(source)
        kinds |= batch_kinds
    assert kinds == {0, iu.FROM_TRACKER, iu.FROM_UAV, iu.FROM_PREDICTION}


def test_five_kinds_of_path_in_one_batch_and_the_invalid_ones(gpu_ctx):
    nan = float("nan")
    rows = [dict(tracker=1, age=0.1, uav=1, dont=1, offset=0.9, n_wp=3, n_pred=iu.N_PRED),        # dont_prepend
            dict(tracker=0, age=0.0, uav=1, dont=0, offset=0.0, n_wp=1, n_pred=0),                 # before takeoff
            dict(tracker=1, age=0.1, uav=1, dont=0, offset=0.1, n_wp=2, n_pred=iu.N_PRED),        # the tracker command
            dict(tracker=1, age=0.1, uav=0, dont=0, offset=iu.offset_at_k(9), n_wp=1, n_pred=iu.N_PRED),   # from the future
            dict(tracker=1, age=0.1, uav=0, dont=0, offset=30.0, n_wp=4, n_pred=iu.N_PRED),       # beyond the horizon
            dict(tracker=1, age=0.1, uav=1, dont=0, offset=nan, n_wp=2, n_pred=iu.N_PRED),
            dict(tracker=1, age=nan, uav=1, dont=0, offset=0.5, n_wp=2, n_pred=iu.N_PRED),
            dict(tracker=1, age=0.1, uav=1, dont=0, offset=0.5, n_wp=2, n_pred=PRED_CAP + 1),
            dict(tracker=1, age=0.1, uav=1, dont=0, offset=0.5, n_wp=2, n_pred=-1),
            dict(tracker=0, age=nan, uav=0, dont=0, offset=0.5, n_wp=2, n_pred=PRED_CAP)]          # nothing to start from
    pred, tracker, uav, decision, k, initial = _run_initial_condition(gpu_ctx, rows, np.random.default_rng(12))
    T, U, F = iu.PREPEND | iu.FROM_TRACKER, iu.PREPEND | iu.FROM_UAV, iu.PREPEND | iu.FROM_FUTURE | iu.FROM_PREDICTION
    assert decision.tolist() == [iu.DROP_FIRST, U, T, F, T | iu.DROP_FIRST, iu.INVALID, iu.INVALID, iu.INVALID, iu.INVALID,
                                 iu.DROP_FIRST]
    assert k.tolist() == [0, 0, 0, 9, 76, 0, 0, 0, 0, 0]
    want1 = np.zeros((4, 4))
    want1[0] = uav[1]
    want1[0, 2] = uav[1, 2] + 1.5
    assert _bits(initial[1]) == _bits(want1) and _bits(initial[2]) == _bits(tracker[2]) and _bits(initial[4]) == _bits(tracker[4])
    assert _bits(initial[3]) == _bits(np.array([a[3, 9] for a in pred]))
    assert not initial[[0, 5, 6, 7, 8, 9]].any()


PREPEND_COUNTS = [0, 1, 2, 5, 1, 0, 2, 3, 1, 0, 2, 4]
PREPEND_WORDS = [iu.PREPEND | iu.FROM_UAV, iu.PREPEND | iu.FROM_TRACKER, iu.PREPEND | iu.FROM_TRACKER | iu.DROP_FIRST, iu.DROP_FIRST,
                 0, 0, 0, iu.PREPEND | iu.FROM_FUTURE | iu.FROM_PREDICTION | iu.DROP_FIRST, iu.DROP_FIRST, iu.DROP_FIRST,
                 iu.INVALID, iu.PREPEND | iu.FROM_UAV]


def _prepend_inputs():
    rng = np.random.default_rng(21)
    vo = np.concatenate([[0], np.cumsum(PREPEND_COUNTS)]).astype(np.int32)
    wp = rng.uniform(-9.0, 9.0, (int(vo[-1]), 4))
    stop = rng.integers(0, 2, int(vo[-1])).astype(np.uint8)
    initial = rng.uniform(-9.0, 9.0, (len(PREPEND_COUNTS), 4, 4))
    return vo, wp, stop, np.array(PREPEND_WORDS, dtype=np.int32), initial


def test_prepend_against_the_numpy_restatement(gpu_ctx):
    vo, wp, stop, words, initial = _prepend_inputs()
    P, n_v, guard = len(PREPEND_COUNTS), wp.shape[0], 4
    off_w, rows_w, stop_w, source_w = iu.prepend_numpy(vo, wp, stop, words, initial)
    assert 0 in np.diff(off_w) and 1 in np.diff(off_w) and 2 in np.diff(off_w)      # paths of 0, 1 and 2 vertices come out
    offsets = torch.full((P + 1 + guard,), -77, dtype=torch.int32, device=DEV)
    rows = torch.full((n_v + P + guard, 4), -77.0, dtype=torch.float64, device=DEV)
    stop_out = torch.full((n_v + P + guard,), 77, dtype=torch.uint8, device=DEV)
    source = torch.full((n_v + P + guard,), -77, dtype=torch.int32, device=DEV)
    plan = _count_plan(gpu_ctx, P)
    try:
        plan.prepend_initial_condition(_dev(vo), _dev(wp), _dev(words), _dev(initial), offsets, rows, stop_at=_dev(stop),
                                       stop_at_out=stop_out, source=source)
        gpu_ctx.synchronize()
    finally:
        plan.close()
    total = int(off_w[-1])
    assert np.array_equal(offsets.cpu().numpy()[:P + 1], off_w) and np.all(offsets.cpu().numpy()[P + 1:] == -77)
    assert _bits(rows.cpu().numpy()[:total]) == _bits(rows_w) and np.all(rows.cpu().numpy()[total:] == -77.0)
    assert np.array_equal(stop_out.cpu().numpy()[:total], stop_w) and np.all(stop_out.cpu().numpy()[total:] == 77)
    assert np.array_equal(source.cpu().numpy()[:total], source_w) and np.all(source.cpu().numpy()[total:] == -77)


def _splice_batch(n, k, cap, rng):
    """six paths at one capacity: the case, a dead path, the case again, a sampler overflow, a path that needs no splice (an old
    prediction) and one whose prediction is shorter than k"""
    P = 6
    n_in = np.array([n, n, n, cap + 1, min(n, cap), n], dtype=np.int32)
    status = np.array([1, 0, 3, 1, 1, 1], dtype=np.int32)
    words = np.full(P, iu.PREPEND | iu.FROM_FUTURE | iu.FROM_PREDICTION, dtype=np.int32)
    ks = np.full(P, k, dtype=np.int32)
    age = np.array([0.005, 0.005, 0.0, 0.005, 0.2 * k + 0.5, 0.005])     # below 0.01 s the prediction's current index is 0
    n_pred = np.array([PRED_CAP, PRED_CAP, k, PRED_CAP, PRED_CAP, k - 1], dtype=np.int32)
    samples = rng.uniform(-9.0, 9.0, (P, cap, 4))
    pos = rng.uniform(100.0, 200.0, (P, PRED_CAP, 4))
    return n_in, status, words, ks, age, n_pred, samples, pos


def _guarded(a, guard=8):
    """a device copy of `a` in the middle of a larger block of sentinels -> (block, view)"""
    block = torch.full((a.size + 2 * guard,), -77.0, dtype=torch.float64, device=DEV)
    view = block[guard:guard + a.size].view(a.shape)
    view.copy_(_dev(a))
    return block, view


def test_splice_grid_against_the_host_splice(gpu_ctx):
    rng = np.random.default_rng(31)
    plan = _count_plan(gpu_ctx, 6)
    try:
        for n, k, cap in iu.splice_cases():
            n_in, status, words, ks, age, n_pred, samples, pos = _splice_batch(n, k, cap, rng)
            args = [_dev(x) for x in (words, ks, age, pos, n_pred)]
            outs = []
            for in_place in (False, False, True):
                block, view = _guarded(samples)
                n_out = torch.full((6,), -5, dtype=torch.int32, device=DEV)
                st_out = torch.full((6,), -5, dtype=torch.int32, device=DEV)
                if in_place:
                    n_out.copy_(_dev(n_in))
                    plan.splice_prediction(view, n_out, *args, status=_dev(status), status_out=st_out)
                    got_block, got = block, view
                else:
                    got_block, got = _guarded(samples)          # what a path that is left alone would hold in place
                    plan.splice_prediction(view, _dev(n_in), *args, samples_out=got, n_samples_out=n_out, status=_dev(status),
                                           status_out=st_out)
                    assert _bits(view.cpu().numpy()) == _bits(samples)
                gpu_ctx.synchronize()
                outs.append((got.cpu().numpy(), n_out.cpu().numpy(), st_out.cpu().numpy(), got_block.cpu().numpy()))
            for got, n_out, st_out, block in outs:
                assert _bits(got) == _bits(outs[0][0]) and np.array_equal(n_out, outs[0][1]) and np.array_equal(st_out, outs[0][2])
                assert np.all(block[:8] == -77.0) and np.all(block[-8:] == -77.0)
            got, n_out, st_out, _ = outs[0]
            pred = dict(position=pos[0], velocity=pos[0], acceleration=pos[0], jerk=pos[0])
            for p in (0, 2):
                pred = {key: pos[p, :n_pred[p]] for key in ("position", "velocity", "acceleration", "jerk")}
                if n + k <= cap:
                    want = api.splice_prediction(pred, k, float(age[p]), samples[p, :n], sample_capacity=cap)
                    assert n_out[p] == n + k and _bits(got[p, :n + k]) == _bits(want), (n, k, cap, p)
                    assert _bits(got[p, n + k:]) == _bits(samples[p, n + k:])          # no row at or behind the new count
                else:
                    with pytest.raises(api.MrsTgError, match="need a capacity of %d" % (n + k)):
                        api.splice_prediction(pred, k, float(age[p]), samples[p, :n], sample_capacity=cap)
                    assert n_out[p] == n + k and _bits(got[p]) == _bits(samples[p]), (n, k, cap, p)
            # left alone, rows and count: the dead path, the sampler overflow, the path whose prediction is too old to matter
            assert n_out[[1, 3, 4, 5]].tolist() == n_in[[1, 3, 4, 5]].tolist()
            assert all(_bits(got[p]) == _bits(samples[p]) for p in (1, 3, 4, 5))
            assert api.splice_prediction({key: pos[4] for key in pred}, k, float(age[4]), samples[4, :n_in[4]]).shape[0] == n_in[4]
            assert st_out.tolist() == [1, 0, 3, 1, 1, -2], st_out     # a prediction shorter than k is flagged, which the host refuses
            with pytest.raises(api.MrsTgError, match="fewer samples"):
                api.splice_prediction({key: pos[5, :k - 1] for key in pred}, k, float(age[5]), samples[5, :n])
    finally:
        plan.close()


def _splice_torch(samples, pos, n_eff, k_eff):
    """the splice as an index restatement: rows 0 .. k-1 of the prediction, then rows 0 .. n-1 of the samples, zeros behind"""
    out = torch.zeros_like(samples)
    for p in range(samples.shape[0]):
        out[p, :k_eff[p]] = pos[p, :k_eff[p]]
        out[p, k_eff[p]:k_eff[p] + n_eff[p]] = samples[p, :n_eff[p]]
    return out


def test_splice_backward_against_torch_autograd(gpu_ctx):
    rng = np.random.default_rng(41)
    cap = 200
    #            spliced       spliced   too long  dead  no splice  overflow  short
    n_in = np.array([65, 129, 150, 40, 70, cap + 1, 30], dtype=np.int32)
    ks = np.array([64, 2, 65, 5, 6, 3, 9], dtype=np.int32)
    status = np.array([1, 4, 1, -1, 1, 1, 1], dtype=np.int32)
    age = np.array([0.05, 0.05, 0.05, 0.05, 9.0, 0.05, 0.05])
    n_pred = np.array([PRED_CAP, PRED_CAP, PRED_CAP, PRED_CAP, PRED_CAP, PRED_CAP, 8], dtype=np.int32)
    n_eff = [65, 129, 150, 0, 70, cap, 30]
    k_eff = [64, 2, 0, 0, 0, 0, 0]
    P = n_in.size
    words = np.full(P, iu.PREPEND | iu.FROM_FUTURE | iu.FROM_PREDICTION, dtype=np.int32)
    up = _dev(rng.integers(-128, 129, (P, cap, 4)) / 64.0)
    s = _dev(rng.uniform(-9, 9, (P, cap, 4))).requires_grad_()
    pos = _dev(rng.uniform(-9, 9, (P, PRED_CAP, 4))).requires_grad_()
    want_s, want_p = torch.autograd.grad((_splice_torch(s, pos, n_eff, k_eff) * up).sum(), (s, pos))
    gs = torch.full_like(s, float("nan"))
    gp = torch.full_like(pos, float("nan"))
    plan = _count_plan(gpu_ctx, P)
    try:
        plan.splice_prediction_vjp(_dev(n_in), _dev(words), _dev(ks), _dev(age), _dev(n_pred), up, gs, gp, status=_dev(status))
        gpu_ctx.synchronize()
        assert torch.equal(gs, want_s) and torch.equal(gp, want_p)
        # and through the autograd function, whose forward is the restatement
        s2, pos2 = s.detach().clone().requires_grad_(), pos.detach().clone().requires_grad_()
        out, n_out, st_out = ag.splice_prediction(plan, s2, _dev(n_in), _dev(words), _dev(ks), _dev(age), pos2, _dev(n_pred),
                                                  status=_dev(status))
        assert torch.equal(out, _splice_torch(s, pos, n_eff, k_eff).detach())
        assert n_out.tolist() == [129, 131, 215, 40, 70, cap + 1, 30] and st_out.tolist() == [1, 4, 1, -1, 1, 1, -2]
        got_s, got_p = torch.autograd.grad((out * up).sum(), (s2, pos2))
        assert torch.equal(got_s, want_s) and torch.equal(got_p, want_p)
    finally:
        plan.close()


def test_initial_condition_backward_against_torch_autograd(gpu_ctx):
    rng = np.random.default_rng(51)
    words = np.array([iu.PREPEND | iu.FROM_TRACKER, iu.PREPEND | iu.FROM_UAV, iu.PREPEND | iu.FROM_FUTURE | iu.FROM_PREDICTION,
                      iu.DROP_FIRST, iu.INVALID, iu.PREPEND | iu.FROM_FUTURE | iu.FROM_PREDICTION | iu.DROP_FIRST,
                      iu.PREPEND | iu.FROM_TRACKER | iu.DROP_FIRST], dtype=np.int32)
    ks = np.array([0, 0, 7, 0, 0, PRED_CAP - 1, 76], dtype=np.int32)
    P = words.size
    up = _dev(rng.integers(-128, 129, (P, 4, 4)) / 64.0)
    tracker = _dev(rng.uniform(-9, 9, (P, 4, 4))).requires_grad_()
    uav = _dev(rng.uniform(-9, 9, (P, 4))).requires_grad_()
    pred = [_dev(rng.uniform(-9, 9, (P, PRED_CAP, 4))).requires_grad_() for _ in range(4)]
    blocks = []
    for p in range(P):
        if words[p] & iu.FROM_TRACKER:
            blocks.append(tracker[p])
        elif words[p] & iu.FROM_UAV:
            blocks.append(torch.cat([(uav[p] + torch.tensor([0.0, 0.0, 1.5, 0.0], dtype=torch.float64, device=DEV))[None],
                                     torch.zeros((3, 4), dtype=torch.float64, device=DEV)]))
        elif words[p] & iu.FROM_PREDICTION:
            blocks.append(torch.stack([a[p, ks[p]] for a in pred]))
        else:
            blocks.append(torch.zeros((4, 4), dtype=torch.float64, device=DEV) * tracker[p])
    want = torch.autograd.grad((torch.stack(blocks) * up).sum(), [tracker, uav] + pred)
    gt = torch.full((P, 4, 4), float("nan"), dtype=torch.float64, device=DEV)
    gu = torch.full((P, 4), float("nan"), dtype=torch.float64, device=DEV)
    gp = [torch.full((P, PRED_CAP, 4), float("nan"), dtype=torch.float64, device=DEV) for _ in range(4)]
    plan = _count_plan(gpu_ctx, P)
    try:
        plan.initial_condition_vjp(_dev(words), _dev(ks), up, gt, gu, gp)
        gpu_ctx.synchronize()
    finally:
        plan.close()
    for got, w in zip([gt, gu] + gp, want):
        assert torch.equal(got, w)
    assert torch.equal(gp[0][5, PRED_CAP - 1], up[5, 0]) and torch.equal(gp[3][2, 7], up[2, 3])


def test_prepend_backward_against_torch_autograd(gpu_ctx):
    vo, wp, stop, words, initial = _prepend_inputs()
    P = len(PREPEND_COUNTS)
    off_w, rows_w, _, source_w = iu.prepend_numpy(vo, wp, stop, words, initial)
    rng = np.random.default_rng(61)
    up = _dev(rng.integers(-128, 129, rows_w.shape) / 64.0)
    w = _dev(wp).requires_grad_()
    ini = _dev(initial).requires_grad_()
    path_of_row = np.repeat(np.arange(P), np.diff(off_w))
    rows = torch.stack([w[v] if v >= 0 else ini[p, 0] for v, p in zip(source_w.tolist(), path_of_row.tolist())])
    assert _bits(rows.detach().cpu().numpy()) == _bits(rows_w)
    want_w, want_i = torch.autograd.grad((rows * up).sum(), (w, ini))
    gw = torch.full_like(w, float("nan"))
    row = torch.full((P, 4), float("nan"), dtype=torch.float64, device=DEV)
    plan = _count_plan(gpu_ctx, P)
    try:
        plan.prepend_initial_condition_vjp(_dev(vo), _dev(words), _dev(off_w), up, gw, row)
        gpu_ctx.synchronize()
        assert torch.equal(gw, want_w) and torch.equal(row, want_i[:, 0]) and not want_i[:, 1:].any()
        w2, ini2 = w.detach().clone().requires_grad_(), ini.detach().clone().requires_grad_()
        out, stop_out, source, offsets = ag.prepend_initial_condition(plan, w2, ini2, _dev(vo), _dev(words), stop_at=_dev(stop))
        assert _bits(out.detach().cpu().numpy()) == _bits(rows_w) and np.array_equal(source.cpu().numpy(), source_w)
        got_w, got_i = torch.autograd.grad((out * up).sum(), (w2, ini2))
        assert torch.equal(got_w, want_w) and torch.equal(got_i, want_i)
    finally:
        plan.close()


def test_chain_from_the_initial_condition_to_a_loss_on_the_spliced_rows(gpu_ctx):
    """initial_condition -> prepend -> solve -> sample -> splice -> loss through autograd, against the same chain cut at the three
    new steps with their backward passes called by hand: bit for bit, since the new passes only copy."""
    rng = np.random.default_rng(71)
    cap, takeoff = 512, 1.5
    rows = [dict(tracker=1, age=0.1, uav=0, dont=0, offset=iu.offset_at_k(5), n_wp=3, n_pred=iu.N_PRED),   # from the future
            dict(tracker=1, age=0.1, uav=1, dont=0, offset=0.0, n_wp=2, n_pred=iu.N_PRED),                 # the tracker command
            dict(tracker=0, age=0.0, uav=1, dont=0, offset=0.0, n_wp=2, n_pred=0),                         # before takeoff
            dict(tracker=1, age=0.1, uav=0, dont=0, offset=iu.offset_at_k(4), n_wp=1, n_pred=iu.N_PRED)]   # one goal waypoint
    P = len(rows)
    vo = np.concatenate([[0], np.cumsum([r["n_wp"] for r in rows])]).astype(np.int32)
    wp_np = np.cumsum(rng.uniform(1.5, 3.0, (int(vo[-1]), 4)), axis=0)
    wp_np[:, 3] = rng.uniform(-0.3, 0.3, int(vo[-1]))
    pred_np = [rng.uniform(-1.0, 1.0, (P, PRED_CAP, 4)) for _ in range(4)]
    pred_np[0][:, :, :3] = np.cumsum(np.full((P, PRED_CAP, 3), 0.2), axis=1)
    tracker_np = rng.uniform(-1.0, 1.0, (P, 4, 4))
    uav_np = rng.uniform(-1.0, 1.0, (P, 4))
    flags = _dev(np.array([r["tracker"] * iu.FLAG_TRACKER | r["uav"] * iu.FLAG_UAV for r in rows], dtype=np.int32))
    t_age, offs = _dev(np.array([r["age"] for r in rows])), _dev(np.array([r["offset"] for r in rows]))
    n_pred, age = _dev(np.array([r["n_pred"] for r in rows], dtype=np.int32)), _dev(np.full(P, 0.05))
    weights = _dev(rng.integers(-128, 129, (P, cap, 4)) / 64.0)
    plan0 = _count_plan(gpu_ctx, P)
    plans = [plan0]

    def leaves():
        return (_dev(tracker_np).requires_grad_(), _dev(uav_np).requires_grad_(), [_dev(a).requires_grad_() for a in pred_np],
                _dev(wp_np).requires_grad_())

    def middle(plan1, wp1, initial, off_h):
        """vertices, solve and sampler of the edited batch: position at every vertex, the state's derivatives at the first one,
        zeros at the last"""
        first, last = off_h[:-1], off_h[1:] - 1
        n_v = int(off_h[-1])
        mask = torch.zeros((n_v, 5), dtype=torch.uint8, device=DEV)
        mask[:, 0] = 1
        mask[first, 1:] = 1
        mask[last, 1:] = 1
        sel = torch.zeros((n_v, P), dtype=torch.float64, device=DEV)
        sel[first, torch.arange(P)] = 1.0
        fv = torch.zeros((n_v, 5, 4), dtype=torch.float64, device=DEV)
        fv = torch.cat([wp1[:, None, :], torch.einsum("vp,pkd->vkd", sel, initial[:, 1:]), fv[:, :1]], dim=1)
        times = (wp1[1:, :3] - wp1[:-1, :3]).detach().norm(dim=1)
        keep = np.ones(n_v - 1, dtype=bool)
        keep[last[:-1]] = False
        times = times[torch.from_numpy(keep).to(DEV)] + 0.5
        coeffs, _, status = ag.solve(plan1, mask, fv, times)
        samples, n = ag.sample(plan1, coeffs, times, 0.2, cap, status)
        return samples, n, status

    try:
        # (1) autograd all the way
        tracker, uav, pred, wp = leaves()
        initial, dec, k = ag.initial_condition(plan0, flags, tracker, t_age, uav, takeoff, offs, _dev(vo), pred, n_pred)
        assert dec.tolist() == [iu.PREPEND | iu.FROM_FUTURE | iu.FROM_PREDICTION | iu.DROP_FIRST, iu.PREPEND | iu.FROM_TRACKER,
                                iu.PREPEND | iu.FROM_UAV, iu.PREPEND | iu.FROM_FUTURE | iu.FROM_PREDICTION]
        wp1, _, _, offsets = ag.prepend_initial_condition(plan0, wp, initial, _dev(vo), dec)
        off_h = offsets.cpu().numpy().astype(np.int64)
        assert np.diff(off_h).tolist() == [3, 3, 3, 2]
        plan1 = api.Plan(gpu_ctx, (off_h - np.arange(P + 1)).astype(np.int32))
        plans.append(plan1)
        samples, n, status = middle(plan1, wp1, initial, off_h)
        assert bool((status > 0).all())
        spliced, n_out, st_out = ag.splice_prediction(plan1, samples, n, dec, k, age, pred[0], n_pred, status=status)
        assert (n_out - n).tolist() == [5, 0, 0, 4] and bool((n_out <= cap).all()) and bool((st_out > 0).all())
        (spliced * weights).sum().backward()
        auto = [tracker.grad, uav.grad, wp.grad] + [a.grad for a in pred]
        assert all(g is not None for g in auto) and all(bool(g.abs().sum() > 0) for g in auto[:4])

        # (2) the same chain, cut at the new steps
        tracker, uav, pred, wp = leaves()
        det = [a.detach() for a in pred]
        initial2 = torch.empty((P, 4, 4), dtype=torch.float64, device=DEV)
        dec2 = torch.empty(P, dtype=torch.int32, device=DEV)
        k2 = torch.empty(P, dtype=torch.int32, device=DEV)
        plan0.initial_condition(flags, tracker.detach(), t_age, uav.detach(), takeoff, offs, _dev(vo), det, n_pred, dec2, k2, initial2)
        assert torch.equal(initial2, initial.detach()) and torch.equal(dec2, dec) and torch.equal(k2, k)
        n_v = wp.shape[0]
        wp1_buf = torch.empty((n_v + P, 4), dtype=torch.float64, device=DEV)
        offsets2 = torch.empty(P + 1, dtype=torch.int32, device=DEV)
        plan0.prepend_initial_condition(_dev(vo), wp.detach(), dec2, initial2, offsets2, wp1_buf)
        assert torch.equal(offsets2, offsets)
        wp1_leaf = wp1_buf[:int(off_h[-1])].clone().requires_grad_()
        initial_leaf = initial2.clone().requires_grad_()
        samples2, n2, status2 = middle(plan1, wp1_leaf, initial_leaf, off_h)
        assert torch.equal(samples2, samples.detach()) and torch.equal(n2, n)
        g_samples = torch.empty_like(samples2)
        g_pos = torch.empty((P, PRED_CAP, 4), dtype=torch.float64, device=DEV)
        plan1.splice_prediction_vjp(n2, dec2, k2, age, n_pred, weights, g_samples, g_pos, status=status2)
        g_wp1, g_initial = torch.autograd.grad(samples2, (wp1_leaf, initial_leaf), grad_outputs=g_samples)
        g_wp = torch.empty((n_v, 4), dtype=torch.float64, device=DEV)
        g_row = torch.empty((P, 4), dtype=torch.float64, device=DEV)
        plan0.prepend_initial_condition_vjp(_dev(vo), dec2, offsets2, g_wp1.contiguous(), g_wp, g_row)
        g_initial = g_initial.clone()
        g_initial[:, 0] += g_row
        g_tracker = torch.empty((P, 4, 4), dtype=torch.float64, device=DEV)
        g_uav = torch.empty((P, 4), dtype=torch.float64, device=DEV)
        g_pred = [torch.empty((P, PRED_CAP, 4), dtype=torch.float64, device=DEV) for _ in range(4)]
        plan0.initial_condition_vjp(dec2, k2, g_initial.contiguous(), g_tracker, g_uav, g_pred)
        gpu_ctx.synchronize()
        hand = [g_tracker, g_uav, g_wp, g_pred[0] + g_pos] + g_pred[1:]
        for a, h in zip(auto, hand):
            assert torch.equal(a, h)
    finally:
        for pl in plans:
            pl.close()

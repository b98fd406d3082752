"""Shared helpers of the sampler's backward-pass tests (test_sample_vjp_host.py, test_gpu_sample_vjp.py): the fixtures, the
CPU harness of csrc/mrs_tg_sample_vjp.hpp, and a torch restatement of the sampled states at given (segment, time) pairs."""
import functools

import numpy as np

from tests import host_harness as hh

load_cases = functools.partial(hh.load_cases, "sample_vjp_cases.json")
load_composite_cases = functools.partial(hh.load_cases, "sample_vjp_composite_cases.json")
build_harness = functools.partial(hh.build, "sample_vjp_harness.cpp")   # (tmp_path, sanitize=False)
N, D, ORDERS = 10, 4, 5


def run_harness(exe, problems, env=None):
    """problems: dicts with seg_times [S], coeffs [S][4][10], dt, capacity, n_orders, grad_states [R][n_orders][4] (R >= the
    number of samples below the capacity; further rows may hold anything), optional status (default 1).
    -> list of dicts n, sample_segment, sample_time, grad_coeffs [S][4][10], grad_seg_times [S]"""
    lines = []
    for p in problems:
        S = len(p["seg_times"])
        G = np.asarray(p["grad_states"], dtype=np.float64).reshape(-1, p["n_orders"], D)
        lines.append("%d %d %d %d %r %s %s %d %s\n" % (S, p["n_orders"], p["capacity"], p.get("status", 1), float(p["dt"]),
                                                        hh.fmt(p["seg_times"]), hh.fmt(p["coeffs"]), G.shape[0], hh.fmt(G)))
    out = hh.run(exe, lines, len(problems), env=env)
    res = []
    for p, line in zip(problems, out):
        S = len(p["seg_times"])
        x = line.split()
        n = int(x[0])
        rows = min(n, p["capacity"])
        assert len(x) == 1 + 2 * rows + S * D * N + S
        pairs = x[1:1 + 2 * rows]
        rest = np.array([float(v) for v in x[1 + 2 * rows:]])
        res.append(dict(n=n, sample_segment=np.array([int(v) for v in pairs[0::2]], dtype=np.int64),
                        sample_time=np.array([float(v) for v in pairs[1::2]]),
                        grad_coeffs=rest[:S * D * N].reshape(S, D, N), grad_seg_times=rest[S * D * N:], raw=line))
    return res


def case_problem(case, pad_rows=0):
    """the harness problem of a fixture; pad_rows NaN rows are appended to the upstream (rows nobody may read)"""
    G = np.asarray(case["grad_states"], dtype=np.float64).reshape(-1, case["n_orders"], D)
    if pad_rows:
        G = np.concatenate([G, np.full((pad_rows, case["n_orders"], D), np.nan)])
    return dict(seg_times=case["seg_times"], coeffs=case["coeffs"], dt=case["dt"], capacity=case["capacity"],
                n_orders=case["n_orders"], grad_states=G)


def fixture_error(case, grad_coeffs, grad_seg_times):
    """|got - fixture| relative to the case's largest gradient entry (a directional case: the three directional derivatives
    relative to the largest of them)"""
    gc = np.asarray(grad_coeffs, dtype=np.float64)
    gt = np.asarray(grad_seg_times, dtype=np.float64)
    if "directions" in case:
        refs = np.array([d["derivative"] for d in case["directions"]])
        got = np.array([np.sum(gc * (np.array(d["d_coeffs_sixteenths"]) / 16.0)) + np.sum(gt * np.array(d["d_seg_times"])) for d in case["directions"]])
        return float(np.max(np.abs(got - refs)) / np.max(np.abs(refs)))
    rc, rt = np.array(case["grad_coeffs"]), np.array(case["grad_seg_times"])
    scale = max(np.max(np.abs(rc)), np.max(np.abs(rt)))
    return float(max(np.max(np.abs(gc - rc)), np.max(np.abs(gt - rt))) / scale)


# ------------------------------------------------------------------------------------------------------------------------
# torch restatement

def states_at(torch, coeffs, seg, t, n_orders=ORDERS):
    """dense float64 Horner: states [K][n_orders][4] of the samples taken in the segments seg [K] (int64 rows of coeffs
    [sum S][4][10]) at the times t [K]; differentiable in coeffs and t.  The heading is NOT wrapped."""
    c = coeffs[seg]   # [K][4][10]
    out = []
    for o in range(n_orders):
        fall = [1.0] * N
        for j in range(N):
            for n in range(o):
                fall[j] *= (j - n)
        acc = c[:, :, N - 1] * fall[N - 1]
        for j in range(N - 2, o - 1, -1):
            acc = acc * t[:, None] + c[:, :, j] * fall[j]
        out.append(acc)
    return torch.stack(out, dim=1)


def sample_times_expr(torch, seg_times, seg_offsets, p_idx, seg_rel, k_index, dt):
    """t_k = k dt - (sum of the times of the path's segments in front of the sample's own), a differentiable expression:
    seg_times [sum S], seg_offsets [P + 1] (CSR), p_idx [K] the sample's path, seg_rel [K] its segment within the path,
    k_index [K] its index in the path (index tensors on seg_times' device).  The sums are taken per path (a difference of
    two entries of one cumulative sum over the whole batch would lose the digits of the batch's total time)."""
    dev = seg_times.device
    so = torch.as_tensor(np.asarray(seg_offsets, dtype=np.int64), device=dev)
    counts = so[1:] - so[:-1]
    cols = torch.arange(int(counts.max()), device=dev)
    inside = cols[None, :] < counts[:, None]
    rows = torch.where(inside, so[:-1, None] + cols[None, :], torch.zeros((), dtype=torch.int64, device=dev))
    Tm = torch.where(inside, seg_times[rows], torch.zeros((), dtype=seg_times.dtype, device=dev))
    before = torch.cumsum(Tm, dim=1) - Tm
    return k_index.to(seg_times.dtype) * dt - before[p_idx, seg_rel]

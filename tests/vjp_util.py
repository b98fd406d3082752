"""Shared helpers of the backward-pass tests (test_vjp_host.py, test_gpu_vjp.py): the fixtures, the CPU harness of
csrc/mrs_tg_vjp.hpp, and a dense float64 torch-autograd restatement of the fixed-times solve.

The restatement solves the whole masked KKT system of a path at once (fixed rows replaced by identity rows, A(T) and Q(T)
formed from their definitions, torch.linalg.solve) and lets torch's autograd differentiate L = sum G . coeffs + g * cost: an
independent route to the same gradients, without the block elimination or the adjoint formulas of the kernel."""
import functools
import math

import numpy as np

from tests import host_harness as hh

load_cases = functools.partial(hh.load_cases, "vjp_cases.json")
load_edge_cases = functools.partial(hh.load_cases, "vjp_edge_cases.json")   # (gen_vjp_cases.py --edges)
build_harness = functools.partial(hh.build, "vjp_harness.cpp")   # (tmp_path, sanitize=False)
N, D, B = 10, 4, 5


def run_harness(exe, problems, env=None):
    """problems: dicts with d, mask [V][5], vals [V][5][4], times [S], coeffs [S][4][10], G ([S][4][10] or None), g.
    -> list of (grad_fixed_values [V][5][4], grad_seg_times [S])"""
    lines = []
    for p in problems:
        S = len(p["times"])
        G = p["G"]
        lines.append("%d %d\n%s\n%s\n%s\n%s\n%d\n%s\n%r\n" % (
            p["d"], S, hh.fmt(p["times"]), " ".join(str(int(x)) for x in np.asarray(p["mask"]).reshape(-1)), hh.fmt(p["vals"]),
            hh.fmt(p["coeffs"]), 0 if G is None else 1, hh.fmt(np.zeros((S, D, N)) if G is None else G), float(p["g"])))
    out = hh.run(exe, lines, 2 * len(problems), env=env)
    res = []
    for i, p in enumerate(problems):
        S = len(p["times"])
        gv = np.array([float(x) for x in out[2 * i].split()]).reshape(S + 1, B, D)
        gt = np.array([float(x) for x in out[2 * i + 1].split()])
        res.append((gv, gt))
    return res


def case_problem(case):
    return dict(d=case["derivative_to_optimize"], mask=np.array(case["fixed_mask"], dtype=np.uint8),
                vals=np.array(case["fixed_values"]), times=np.array(case["seg_times"]), coeffs=np.array(case["coeffs"]),
                G=np.array(case["grad_coeffs"]), g=case["grad_cost"])


def rel_error(got_v, got_t, ref_v, ref_t):
    """max |got - ref| over both gradients, relative to the largest entry of the path's reference gradient"""
    scale = max(np.max(np.abs(ref_v)), np.max(np.abs(ref_t)))
    return max(np.max(np.abs(np.asarray(got_v) - ref_v)), np.max(np.abs(np.asarray(got_t) - ref_t))) / scale


def directional_error(case, got_v, got_t):
    """worst |<grad, direction> - fixture| / sum |grad_i direction_i| over the case's directions"""
    worst = 0.0
    for dr in case["directions"]:
        dt, dv = np.array(dr["d_seg_times"]), np.array(dr["d_fixed_values"])
        val = float(np.sum(got_t * dt) + np.sum(got_v * dv))
        scale = float(np.sum(np.abs(got_t * dt)) + np.sum(np.abs(got_v * dv)))
        worst = max(worst, abs(val - dr["derivative"]) / scale)
    return worst


# ---- dense torch restatement ------------------------------------------------------------------------------------------
def _base(r, k):
    return math.factorial(k) / math.factorial(k - r) if k >= r else 0.0


def _abar_inv():
    import mpmath as mp
    with mp.workdps(40):
        A = mp.matrix(N, N)
        for r in range(B):
            A[r, r] = _base(r, r)
            for k in range(r, N):
                A[B + r, k] = _base(r, k)
        Ai = mp.inverse(A)
        return [[float(Ai[i, j]) for j in range(N)] for i in range(N)]


def dense_solve(mask, vals, times, d, G, g):
    """Paths of one segment count S, batched: mask [P][V][5], vals [P][V][5][4], times [P][S] (float64 torch tensors; vals and
    times may require grad), G [P][S][4][10], g [P].  -> (coeffs [P][S][4][10], cost [P], loss) with autograd graph."""
    import torch
    P, S = times.shape
    V = S + 1
    dt = torch.float64
    # A(T)^-1 = diag(T^-k) Abar^-1 diag(T^s(a)), Abar = A(1) (rows r = p^(r)(0), rows 5 + r = p^(r)(1)), inverted in 40 digits
    kpow = torch.arange(N, dtype=dt)
    Ainv = (times[..., None, None] ** -kpow[:, None]) * torch.tensor(_abar_inv(), dtype=dt) * \
        (times[..., None, None] ** (kpow % B)[None, :])
    Q = torch.zeros(P, S, N, N, dtype=dt)
    for i in range(d, N):
        for j in range(d, N):
            e = i + j - 2 * d + 1
            Q[..., i, j] = 2 * _base(d, i) * _base(d, j) * times ** e / e
    H = Ainv.transpose(-1, -2) @ Q @ Ainv
    n = B * V
    R = torch.zeros(P, n, n, dtype=dt)
    for i in range(S):
        R = R + torch.nn.functional.pad(H[:, i], (B * i, n - B * i - N, B * i, n - B * i - N))
    free = (mask.reshape(P, n) == 0).to(dt)
    fixed = 1.0 - free
    dF = vals.reshape(P, n, D) * fixed[..., None]
    M = free[:, :, None] * R * free[:, None, :] + torch.diag_embed(fixed)
    rhs = dF - free[..., None] * (R @ dF)
    sc = torch.diagonal(M, dim1=-2, dim2=-1).abs().clamp_min(1e-300).rsqrt()   # (Jacobi scaling: the slots differ by T^k)
    dall = sc[..., None] * torch.linalg.solve(sc[:, :, None] * M * sc[:, None, :], sc[..., None] * rhs)
    idx = torch.arange(N)
    U = torch.stack([dall[:, B * i + idx, :] for i in range(S)], 1)   # [P][S][10][4]
    C = (Ainv @ U).transpose(-1, -2)                                   # [P][S][4][10]
    J = 0.5 * torch.einsum("psak,psab,psbk->p", U, H, U)
    L = (G * C).sum() + (g * J).sum()
    return C, J, L


def dense_vjp(mask, vals, times, d, G, g):
    """numpy in, numpy out (one segment count): coeffs [P][S][4][10], cost [P], dL/dvals [P][V][5][4], dL/dtimes [P][S]"""
    import torch
    v = torch.tensor(vals, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(times, dtype=torch.float64, requires_grad=True)
    C, J, L = dense_solve(torch.tensor(mask), v, t, d, torch.tensor(G, dtype=torch.float64), torch.tensor(g, dtype=torch.float64))
    L.backward()
    return C.detach().numpy(), J.detach().numpy(), v.grad.numpy(), t.grad.numpy()
